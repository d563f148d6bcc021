"""Quantized compressors: the counterpart of the reference's
``QuantizedZeroPoint``, ``QuantizedLSTM`` and ``QuantizedFP``
(``sfl/utils/compressor/quantized_compressor.py:65-228``).  A dense float32 /
float64 tensor travels as one int8 (or int16) code per element and a few
host scalars.

The definition.  ``T`` is the data's type, float32 or float64; **every
operation is rounded in T** and ``rint`` is round-half-to-even.  This is the
reference's code as numpy 2 evaluates it (NEP 50: a Python scalar never widens
``T``).  The reference pins numpy 1.23, whose value-based scalar promotion
computes ``scale`` and ``q`` of float32 data in float64: results of the two
numpy generations can differ in the last bit.  ``bits = quant_bits``; the codes
keep the data's shape and are int8 for ``bits <= 8``, int16 for ``bits <= 16``
(int32, int64 beyond, host arrays only): the reference's next recommended
width.

``QuantizedZeroPoint``, with ``mn, mx = min(x), max(x)``,
``qmin = -2^(bits-1)``, ``qmax = 2^(bits-1) - 1``::

    scale = T(mx - mn) / T(qmax - qmin)
    izp   = T(qmin) - T(mn / scale)
    z     = qmin if izp < qmin else qmax if izp > qmax else int(izp)
    code  = int(rint(clip(x / scale + T(z), qmin, qmax)))
    dec   = (T(code) - T(z)) * scale

The division is a true division, never a multiply by a reciprocal.

``QuantizedLSTM``::

    q    = T(2^bits - 1) / T(mx - mn)
    rqm  = int(rint(T(q * mn))) + 2^(bits-1)
    code = sat(rint(q * x) - T(rqm))
    dec  = (T(code) + T(rqm)) / q

**``sat`` clamps to the storage range; this is the first refinement.**  The
reference casts without clamping, and an out-of-range float-to-int8 cast wraps
on x86: the largest element would come back as the smallest.

``QuantizedFP`` at 8 bits, ``(max_value, mant_len, exp_offset)`` = (448, 8, 6)
for E4M3 and (57344, 4, 14) for E5M2::

    a, amax = |x|, max|x|
    scale = T(max_value) / (amax if amax > 0 else T(1))
    m, e  = frexp(a * scale)
    qe    = e + exp_offset if e > -exp_offset else 0
    qm    = rint((2 m - 1) * mant_len)     # may equal mant_len: carries into qe
    code  = sign(x) * (qe * mant_len + qm)                      # int8
    c     = |code| taken in int32
    dec   = sign(code) * ldexp(((c % mant_len) / T(mant_len) + 1) / 2,
                               c // mant_len - exp_offset) / scale

**``c`` is taken in int32, so -128 is 128; this is the second refinement**
(numpy's int8 ``abs`` wraps; ``compress`` never emits -128).  The reference's
treatment of tiny values stays: a scaled magnitude below ``2^-exp_offset`` gets
``qe = 0`` and keeps its mantissa field only, so whatever its exponent was it
decodes into ``[2^-(exp_offset+1), 2^-exp_offset) / scale``, or to 0 when that
field is 0.  ``QuantizedFP`` at 16 / 32 / 64 bits is a cast.

Refusals, ``ValueError`` with the same words on host and device, naming the
entry's position in the list.  Zero-point and LSTM refuse a tensor whose
``scale`` (``mx - mn`` and ``q`` for LSTM) is not finite and positive: a NaN
anywhere (``min`` and ``max`` propagate it, as ``np.min`` / ``np.max``), an
inf, a constant tensor, a single element, an empty tensor, a range so small
that ``q`` overflows.  fp8 refuses a NaN or an inf, and a largest magnitude so
small that ``scale`` overflows; an all-zero tensor is fine (all codes 0).
Integer data raises ``TypeError``; a width outside 1..64 or an fp format other
than E4M3 / E5M2 the reference's ``RuntimeError``.  The reference raises on
all-zero and NaN input and returns garbage for the rest.

Where it runs.  numpy arrays and CPU tensors run numpy.  CUDA float32 / float64
tensors run the ``sa_quant_*`` kernels (``sfl_amd/csrc/sa_quant.hip``) and give
CUDA int8 / int16 codes: the range kernel, one pinned read of its three words,
the parameters **by the function the host form uses**, then the code kernel.
So ``scale``, ``z``, ``q`` and ``rqm`` are host scalars as in the reference, and
host and device can differ only in ``min`` / ``max`` or the per-element kernel.
``decompress`` reads nothing back.  On the device ``quant_bits > 16`` is
refused (host arrays take any width).

``QuantizedKmeans`` (``quantized_compressor.py:231-279``): a 1-D k-means whose
labels are the codes and whose centres ``q`` decode them.  The reference fits
scikit-learn's randomly initialised ``KMeans(K, n_init=1, max_iter=50)``; here
the fit is pinned.  ``n`` is the element count, ``K < n < 2^32``;
``K = n_clusters`` (default ``quant_bits``, as the reference),
``2 <= K <= 2^quant_bits``; ``U = 2^32 - 1``; all integer arithmetic is
unsigned 64-bit and floors.

1. Range and image.  ``mn, mx = min(x), max(x)`` (NaN-propagating).  In
   float64 ``s = U / (mx - mn)`` and ``step = (mx - mn) / U``;
   ``u_i = min(U, uint64(rint((float64(x_i) - float64(mn)) * s)))``, the
   subtraction and the multiplication rounded separately (never an FMA).
2. Start, ``init="cbrt"`` (Panter-Dite: the quantiles of the cube root of the
   density).  ``h[b]`` counts the ``u`` with ``u >> 20 == b``, 4096 bins;
   ``w[b] = icbrt(h[b] << 30)``, the exact integer cube root; ``W`` its
   inclusive prefix sum, ``tot = W[4095]``, ``W[-1] = 0``.  For ``j`` in
   ``0..K-1``: ``r = ((2j+1) * tot) // (2K)``; ``b`` the first bin with
   ``W[b] > r``; ``c_j = (b << 20) + (((r - W[b-1]) << 20) // w[b])``
   (``kmeans_init(h, K)``, host code for both forms).  ``init`` may also be an
   array of ``K`` non-decreasing centres of type ``T``, imaged by step 1 and
   clipped to ``[0, U]`` (a warm start).  ``init=None`` is refused.
3. Step.  ``b_j = (c_j + c_{j+1}) >> 1``; ``label(u)`` is the number of ``j``
   with ``b_j < u`` (an element on a boundary belongs to the lower cluster);
   ``cnt_j`` and ``sum_j`` run over the labels;
   ``c'_j = sum_j // cnt_j + (2 * (sum_j % cnt_j) >= cnt_j)``; an empty
   cluster keeps ``c_j``.  ``n_iter`` counts steps; the fit stops after the
   step in which ``c' == c`` for all clusters, or after ``max_iter`` steps.
4. Payload.  The labels under the final centres, ``code = label - 2^(bits-1)``
   in the storage type and the data's shape;
   ``q[j] = T(float64(mn) + float64(c_j) * step)``, a host array ``(K, 1)``
   like ``cluster_centers_``; ``KmeansCompressData`` also carries ``n_iter``.
5. ``n <= K`` passes the tensor through (``origin_type=None``, ``q=None``).
   ``decompress`` gives ``q[code + 2^(bits-1)]`` as ``T``; a code outside
   ``[0, K)`` is never used as an index: ``ValueError`` with the least such
   position.

Refused with ``_refuse``'s wording: a NaN, an inf, ``mx - mn`` not finite and
positive in float64 (or so small that ``s`` overflows), an empty tensor.
Refinements against the reference: the deterministic start; the integer image
(float32 values below ``range * 2^-32`` and float64 resolution beyond 32 bits
are lost); ``K > 2^quant_bits`` is refused where the reference wraps the
labels; an empty cluster keeps its centre where scikit-learn relocates it; the
stop is exact where scikit-learn stops at ``tol = 1e-4 * var``.  On the device
(``sa_kmeans_*``, ``sfl_amd/csrc/sa_kmeans.hip``): ``K <= 256``,
``quant_bits <= 16``; three pinned reads (the range, the histogram, the
centres with ``n_iter``), ``max_iter`` steps enqueued back to back; host and
device give the same codes, ``q`` and ``n_iter``.
"""

from __future__ import annotations

import numpy as np
import torch

from .sparse import _host, _np_dtype

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
_STORE = ((8, np.int8), (16, np.int16), (32, np.int32), (64, np.int64))
FP8_FORMATS = {"E4M3": (448, 8, 6), "E5M2": (57344, 4, 14)}  # max_value, mant_len, exp_offset


def _torch_dtype(dt) -> torch.dtype:
    return torch.from_numpy(np.empty(0, dtype=dt)).dtype


class QuantizedCompressedData:
    """One compressed tensor: ``compressed_data`` (the codes, in the data's
    shape: a numpy array, a CPU tensor or a tensor on a GPU), ``quant_bits``
    and ``origin_type`` (the data's numpy dtype); the subclasses add the
    scalars of their scheme, with the reference's field names."""

    _scalars: tuple = ()

    def __init__(self, compressed_data, quant_bits: int, origin_type=None):
        self.compressed_data = compressed_data
        self.quant_bits = quant_bits
        self.origin_type = None if origin_type is None else _np_dtype(origin_type)

    @property
    def nbytes(self) -> int:
        """The codes: what travels besides a few scalars."""
        d = self.compressed_data
        if isinstance(d, torch.Tensor):
            return d.numel() * d.element_size()
        return int(d.nbytes)

    @property
    def is_device(self) -> bool:
        return isinstance(self.compressed_data, torch.Tensor) and self.compressed_data.is_cuda

    def to(self, device):
        """The same object with its codes on ``device`` (a torch device): a
        numpy array on the CPU, a tensor on a GPU.  Host and device exchange
        them through pinned memory (``hostpipe.h2d`` / ``d2h``)."""
        device = torch.device(device)
        if device.type == "cpu":
            codes = _host(self.compressed_data)
        else:
            from .. import hostpipe as H

            codes = H.h2d(self.compressed_data, device)
        return type(self)(codes, self.quant_bits, self.origin_type, *(getattr(self, s) for s in self._scalars))

    def __repr__(self):
        d = self.compressed_data
        where = str(d.device) if isinstance(d, torch.Tensor) else "host"
        return f"{type(self).__name__}(shape={tuple(d.shape)}, quant_bits={self.quant_bits}, {where})"


class ZeroPointCompressData(QuantizedCompressedData):
    _scalars = ("scale", "nudged_zero_point")

    def __init__(self, compressed_data, quant_bits, origin_type, scale, nudged_zero_point):
        super().__init__(compressed_data, quant_bits, origin_type)
        self.scale = scale
        self.nudged_zero_point = nudged_zero_point


class LSTMCompressData(QuantizedCompressedData):
    _scalars = ("q", "rqm")

    def __init__(self, compressed_data, quant_bits, origin_type, q, rqm):
        super().__init__(compressed_data, quant_bits, origin_type)
        self.q = q
        self.rqm = rqm


class FPCompressData(QuantizedCompressedData):
    _scalars = ("scale",)

    def __init__(self, compressed_data, quant_bits, origin_type, scale=None):
        super().__init__(compressed_data, quant_bits, origin_type)
        self.scale = scale


# ---------------------------------------------------------------------------
# the scalars: one function per scheme, for the host and the device form
# ---------------------------------------------------------------------------
def _refuse(name: str, why: str) -> ValueError:
    return ValueError(f"quantized entry {name}: {why}")


def zero_point_params(mn, mx, bits: int, name: str = "[0]"):
    """``(scale, z)`` from ``min`` and ``max`` (numpy scalars of the data's type)."""
    T = mn.dtype.type
    qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    with np.errstate(all="ignore"):
        scale = T(mx - mn) / T(qmax - qmin)
        if not (np.isfinite(scale) and scale > 0):
            raise _refuse(name, "the scale (max - min) / (qmax - qmin) is not finite and positive: a NaN, an inf, "
                                "a constant tensor, a single element or no element at all")
        izp = T(qmin) - T(mn / scale)
    z = qmin if izp < qmin else qmax if izp > qmax else int(izp)
    return scale, z


def lstm_params(mn, mx, bits: int, name: str = "[0]"):
    """``(q, rqm)`` from ``min`` and ``max`` (numpy scalars of the data's type)."""
    T = mn.dtype.type
    with np.errstate(all="ignore"):
        width = T(mx - mn)
        q = T((1 << bits) - 1) / width
        if not (np.isfinite(width) and width > 0 and np.isfinite(q)):
            raise _refuse(name, "the range max - min is not finite and positive, or too small to divide by: a NaN, "
                                "an inf, a constant tensor, a single element or no element at all")
        rqm = int(np.rint(T(q * mn))) + (1 << (bits - 1))
    return q, rqm


def fp8_scale(amax, max_value: int, name: str = "[0]"):
    """``scale`` from ``max|x|`` (a numpy scalar of the data's type)."""
    T = amax.dtype.type
    with np.errstate(all="ignore"):
        scale = T(max_value) / (amax if amax > 0 else T(1))
        if not (np.isfinite(amax) and np.isfinite(scale)):
            raise _refuse(name, "the largest magnitude is NaN, inf, or too small to scale to the fp8 range")
    return scale


def _store_type(bits: int):
    for width, t in _STORE:
        if bits <= width:
            return t
    raise RuntimeError(f"Unknown input quant_bits {bits}")


def _store_range(T, store):
    """The storage range as two T that the cast back to ``store`` cannot leave."""
    info = np.iinfo(store)
    lo, hi = T(info.min), T(info.max)
    if int(hi) > info.max:  # T rounded 2^k - 1 up to 2^k
        hi = np.nextafter(hi, T(0))
    return lo, hi


# ---------------------------------------------------------------------------
# where a tensor lives
# ---------------------------------------------------------------------------
def _float_type(x, name: str, who: str, floats=_FLOATS) -> np.dtype:
    dt = _np_dtype(x.dtype)
    if dt not in floats:
        raise TypeError(f"{who}: entry {name} is {dt}; float32 or float64 data")
    return dt


def _range_device(flat: torch.Tensor):
    """``(min, max, max|x|)`` of a flat device tensor as numpy scalars: the
    range kernel and one pinned read of its three words."""
    from .. import hostpipe as H
    from .. import kernels as K
    from .compressor import _scratch_for

    out3 = torch.empty(3, dtype=flat.dtype, device=flat.device)
    K.quant_range(flat, _scratch_for(flat, K.quant_scratch_bytes(flat.numel(), flat.dtype)), out3)
    w = H.d2h(out3, pooled=False)
    return w[0], w[1], w[2]


def _range_host(flat: np.ndarray):
    T = flat.dtype.type
    if flat.size == 0:
        return T(np.inf), T(-np.inf), T(0)
    with np.errstate(all="ignore"):
        return np.min(flat), np.max(flat), np.max(np.abs(flat))


class _Where:
    """One entry seen as a flat contiguous vector where it lives."""

    def __init__(self, x, name: str, who: str):
        self.shape = tuple(x.shape)
        self.tensor = isinstance(x, torch.Tensor)
        self.device = x.device if self.tensor and x.is_cuda else None
        if not self.tensor:
            x = np.asarray(x)
        self.dtype = _float_type(x, name, who)
        if self.device is not None:
            self.flat = x.detach().contiguous().reshape(-1)
        else:
            self.flat = np.ascontiguousarray(x.detach().numpy() if self.tensor else x).reshape(-1)

    def range(self):
        return _range_device(self.flat) if self.device is not None else _range_host(self.flat)

    def codes(self, store) -> torch.Tensor:
        return torch.empty(self.flat.numel(), dtype=_torch_dtype(store), device=self.device)

    def wrap(self, codes):
        """Host codes as what the entry was; in the entry's shape."""
        codes = codes.reshape(self.shape)
        return torch.from_numpy(codes) if self.tensor and self.device is None else codes


def _codes_of(c: QuantizedCompressedData, store, name: str, who: str):
    """(codes, is_device, was_tensor): the codes flat and contiguous, checked against ``store``."""
    d = c.compressed_data
    if _np_dtype(d.dtype) != np.dtype(store):
        raise ValueError(f"{who}: entry {name} holds {d.dtype} codes; {c.quant_bits} bits are stored as "
                         f"{np.dtype(store).name}")
    if c.origin_type not in _FLOATS:
        raise TypeError(f"{who}: entry {name} has origin_type {c.origin_type}; float32 or float64 data")
    if isinstance(d, torch.Tensor) and d.is_cuda:
        return d.detach().contiguous().reshape(-1), True, True
    if isinstance(d, torch.Tensor):
        return np.ascontiguousarray(d.detach().numpy()).reshape(-1), False, True
    return np.ascontiguousarray(d).reshape(-1), False, False


def _unwrap(dec, shape, was_tensor: bool):
    dec = dec.reshape(shape)
    return torch.from_numpy(dec) if was_tensor and not isinstance(dec, torch.Tensor) else dec


# ---------------------------------------------------------------------------
# the compressors
# ---------------------------------------------------------------------------
class QuantizedCompressor:
    """The reference's ``QuantizedCompressor`` / ``Compressor``: ``compress``
    takes an array (numpy, a CPU tensor or a CUDA tensor) and gives one
    compressed object, or a list / tuple of arrays and gives a list;
    ``decompress`` and ``iscompressed`` take one object or a list."""

    def __init__(self, quant_bits: int = 8):
        self.quant_bits = quant_bits
        self.np_type = self._infer_np_type(quant_bits)

    def _infer_np_type(self, quant_bits):
        if quant_bits <= 0 or quant_bits > 64:
            raise RuntimeError(f"The quantized bits len must be between 0 and 64, got {quant_bits}")
        return _store_type(quant_bits)

    def _device_bits(self, w: _Where, name: str) -> None:
        if w.device is not None and self.quant_bits > 16:
            raise ValueError(f"{type(self).__name__}: entry {name} is a device tensor, which takes quant_bits <= 16 "
                             f"(got {self.quant_bits}); host arrays take any width")

    def compress(self, data, **kwargs):
        if isinstance(data, (np.ndarray, torch.Tensor)):
            return self._compress_one(data, "[0]")
        if not isinstance(data, (list, tuple)):
            raise TypeError(f"invalid data: {type(data)}")
        return [self._compress_one(d, f"[{i}]") for i, d in enumerate(data)]

    def decompress(self, data):
        if not isinstance(data, list):
            return self._decompress_one(data, "[0]")
        return [self._decompress_one(d, f"[{i}]") for i, d in enumerate(data)]

    def iscompressed(self, data):
        if not isinstance(data, list):
            return isinstance(data, QuantizedCompressedData)
        return [isinstance(x, QuantizedCompressedData) for x in data]


class QuantizedZeroPoint(QuantizedCompressor):
    """The reference's ``QuantizedZeroPoint`` (arXiv:1712.05877); the module's
    docstring has the definition."""

    ZeroPointCompressData = ZeroPointCompressData

    def _compress_one(self, data, name="[0]"):
        from .._lib import SA_QUANT_ZERO_POINT

        bits, w = self.quant_bits, _Where(data, name, "QuantizedZeroPoint")
        self._device_bits(w, name)
        T = w.dtype.type
        mn, mx, _ = w.range()
        scale, z = zero_point_params(mn, mx, bits, name)
        qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        if w.device is not None:
            from .. import kernels as K

            codes = K.quant_affine(w.flat, SA_QUANT_ZERO_POINT, float(scale), float(z), qmin, qmax,
                                   w.codes(self.np_type)).reshape(w.shape)
        else:
            with np.errstate(all="ignore"):
                v = np.clip(w.flat / scale + T(z), T(qmin), T(qmax))
                codes = w.wrap(np.rint(v).astype(self.np_type))
        return ZeroPointCompressData(codes, bits, w.dtype, scale, z)

    def _decompress_one(self, c, name="[0]"):
        from .._lib import SA_QUANT_ZERO_POINT

        codes, on_device, was_tensor = _codes_of(c, _store_type(c.quant_bits), name, "QuantizedZeroPoint")
        T = c.origin_type.type
        scale, z = T(c.scale), T(c.nudged_zero_point)
        if on_device:
            from .. import kernels as K

            out = torch.empty(codes.numel(), dtype=_torch_dtype(c.origin_type), device=codes.device)
            dec = K.dequant_affine(codes, SA_QUANT_ZERO_POINT, float(scale), float(z), out)
        else:
            dec = (codes.astype(T) - z) * scale
        return _unwrap(dec, tuple(c.compressed_data.shape), was_tensor)


class QuantizedLSTM(QuantizedCompressor):
    """The reference's ``QuantizedLSTM`` (arXiv:1607.04683) with codes that
    saturate; the module's docstring has the definition."""

    LSTMCompressData = LSTMCompressData

    def _compress_one(self, data, name="[0]"):
        from .._lib import SA_QUANT_LSTM

        bits, w = self.quant_bits, _Where(data, name, "QuantizedLSTM")
        self._device_bits(w, name)
        T = w.dtype.type
        mn, mx, _ = w.range()
        q, rqm = lstm_params(mn, mx, bits, name)
        with np.errstate(all="ignore"):
            rqm_t = T(rqm)
        if w.device is not None:
            from .. import kernels as K

            info = np.iinfo(self.np_type)
            codes = K.quant_affine(w.flat, SA_QUANT_LSTM, float(q), float(rqm_t), int(info.min), int(info.max),
                                   w.codes(self.np_type)).reshape(w.shape)
        else:
            lo, hi = _store_range(T, self.np_type)
            with np.errstate(all="ignore"):
                v = np.clip(np.rint(q * w.flat) - rqm_t, lo, hi)
                codes = w.wrap(v.astype(self.np_type))
        return LSTMCompressData(codes, bits, w.dtype, q, rqm)

    def _decompress_one(self, c, name="[0]"):
        from .._lib import SA_QUANT_LSTM

        codes, on_device, was_tensor = _codes_of(c, _store_type(c.quant_bits), name, "QuantizedLSTM")
        T = c.origin_type.type
        with np.errstate(all="ignore"):
            q, rqm_t = T(c.q), T(c.rqm)
        if on_device:
            from .. import kernels as K

            out = torch.empty(codes.numel(), dtype=_torch_dtype(c.origin_type), device=codes.device)
            dec = K.dequant_affine(codes, SA_QUANT_LSTM, float(q), float(rqm_t), out)
        else:
            with np.errstate(all="ignore"):
                dec = (codes.astype(T) + rqm_t) / q
        return _unwrap(dec, tuple(c.compressed_data.shape), was_tensor)


class QuantizedFP(QuantizedCompressor):
    """The reference's ``QuantizedFP`` (arXiv:2209.05433): fp8 codes in int8
    with a scale, or a cast to float16 / 32 / 64."""

    FPCompressData = FPCompressData

    def __init__(self, quant_bits: int = 8, format="E4M3"):
        super().__init__(quant_bits)
        if quant_bits not in [8, 16, 32, 64]:
            raise RuntimeError(f"The quantized bits for QuantizedFP must in 8/16/32/64, got {quant_bits}")
        if quant_bits == 8 and format not in FP8_FORMATS:
            raise RuntimeError(f"The format for fp8 quantized must in E4M3/E5M2, got {format}")
        self.format = format
        self.config = dict(zip(("max_value", "mant_len", "exp_offset"), FP8_FORMATS.get(format, FP8_FORMATS["E4M3"])))

    def _cast(self, x, dt: np.dtype, name: str):
        if _np_dtype(x.dtype).kind != "f":
            raise TypeError(f"QuantizedFP: entry {name} is {_np_dtype(x.dtype)}; floating-point data")
        if isinstance(x, torch.Tensor):
            return x.detach().to(_torch_dtype(dt))
        return np.asarray(x).astype(dt)

    def _compress_one(self, data, name="[0]"):
        bits = self.quant_bits
        if bits > 8:
            if not isinstance(data, torch.Tensor):
                data = np.asarray(data)
            return FPCompressData(self._cast(data, np.dtype(f"float{bits}"), name), bits, _np_dtype(data.dtype))
        max_value, ml, off = (self.config[k] for k in ("max_value", "mant_len", "exp_offset"))
        w = _Where(data, name, "QuantizedFP")
        T = w.dtype.type
        scale = fp8_scale(w.range()[2], max_value, name)
        if w.device is not None:
            from .. import kernels as K

            codes = K.quant_fp8(w.flat, float(scale), ml, off, w.codes(np.int8)).reshape(w.shape)
        else:
            x = w.flat
            m, e = np.frexp(np.abs(x) * scale)
            qe = np.where(e > -off, e + off, 0)
            qm = np.rint((T(2) * m - T(1)) * T(ml))
            codes = w.wrap((np.sign(x) * (qe * ml + qm)).astype(np.int8))
        return FPCompressData(codes, bits, w.dtype, scale)

    def _decompress_one(self, c, name="[0]"):
        if c.quant_bits != 8:
            return self._cast(c.compressed_data, c.origin_type, name)
        ml, off = self.config["mant_len"], self.config["exp_offset"]
        codes, on_device, was_tensor = _codes_of(c, np.int8, name, "QuantizedFP")
        T = c.origin_type.type
        scale = T(c.scale)
        if on_device:
            from .. import kernels as K

            out = torch.empty(codes.numel(), dtype=_torch_dtype(c.origin_type), device=codes.device)
            dec = K.dequant_fp8(codes, float(scale), ml, off, out)
        else:
            a = np.abs(codes.astype(np.int32))
            mant = ((a % ml).astype(T) / T(ml) + T(1)) / T(2)
            with np.errstate(all="ignore"):
                dec = np.sign(codes).astype(T) * np.ldexp(mant, a // ml - off) / scale
        return _unwrap(dec, tuple(c.compressed_data.shape), was_tensor)


# ---------------------------------------------------------------------------
# QuantizedKmeans: a pinned 1-D k-means (the module's docstring has the definition)
# ---------------------------------------------------------------------------
KMEANS_U = (1 << 32) - 1  # the image's largest value
KMEANS_BINS, KMEANS_BIN_SHIFT = 4096, 20  # the start's histogram: u >> 20
KMEANS_DEVICE_MAX_K = 256


class KmeansCompressData(QuantizedCompressedData):
    """``q``: the centres, a host array ``(K, 1)`` of the data's type (the
    reference's ``cluster_centers_``); ``n_iter``: the steps the fit took.  A
    tensor that passed through (``n <= K``) has ``origin_type`` and ``q`` None."""

    _scalars = ("q", "n_iter")

    def __init__(self, compressed_data, quant_bits, origin_type=None, q=None, n_iter=0):
        super().__init__(compressed_data, quant_bits, origin_type)
        self.q = q
        self.n_iter = n_iter


def kmeans_scale(mn, mx, name: str = "[0]"):
    """``(mn, s, step)`` as float64 from ``min`` and ``max`` (numpy scalars of the data's type)."""
    with np.errstate(all="ignore"):
        lo, width = np.float64(mn), np.float64(mx) - np.float64(mn)
        s, step = np.float64(KMEANS_U) / width, width / np.float64(KMEANS_U)
        if not (np.isfinite(width) and width > 0 and np.isfinite(s)):
            raise _refuse(name, "the range max - min is not finite and positive, or too small to divide by: a NaN, "
                                "an inf, a constant tensor, a single element or no element at all")
    return lo, s, step


def kmeans_image(x: np.ndarray, mn, s) -> np.ndarray:
    """The image ``u`` of ``x`` as uint64: subtract, multiply, ``rint``, clip to ``U``, each rounded in float64."""
    with np.errstate(all="ignore"):
        v = np.rint((x.astype(np.float64) - mn) * s)
        return np.clip(v, 0.0, np.float64(KMEANS_U)).astype(np.uint64)


def _icbrt(v: np.ndarray) -> np.ndarray:
    """The exact integer cube root of uint64 values below 2^62."""
    w = np.floor(np.cbrt(v.astype(np.float64))).astype(np.uint64)
    w = np.where(w * w * w > v, w - np.uint64(1), w)  # the float root is within one of the integer root
    return np.where((w + np.uint64(1)) ** 3 <= v, w + np.uint64(1), w)


def kmeans_init(h, K: int) -> np.ndarray:
    """The ``"cbrt"`` start from the histogram ``h`` (4096 counts of
    ``u >> 20``): ``K`` sorted centres as uint64, the ``(2j+1) / 2K`` quantiles
    of the cube root of the density, interpolated inside their bin."""
    h = np.asarray(h).astype(np.uint64)
    if h.shape != (KMEANS_BINS,):
        raise ValueError(f"kmeans_init: the histogram has {KMEANS_BINS} bins")
    w = _icbrt(h << np.uint64(30))
    W = np.cumsum(w, dtype=np.uint64)  # below 2^33; (2K - 1) * tot and (r - below) << 20 stay far below 2^64
    r = (np.arange(1, 2 * K, 2, dtype=np.uint64) * W[-1]) // np.uint64(2 * K)
    b = np.searchsorted(W, r, side="right")  # the first bin with W[b] > r
    below = np.where(b > 0, W[np.maximum(b, 1) - 1], np.uint64(0))
    shift = np.uint64(KMEANS_BIN_SHIFT)
    return (b.astype(np.uint64) << shift) + ((r - below) << shift) // w[b]


def kmeans_update(c: np.ndarray, cnt: np.ndarray, total: np.ndarray) -> np.ndarray:
    """``c'``: every cluster's sum over its count, rounded half up; an empty cluster keeps its centre."""
    one = np.maximum(cnt, np.uint64(1))
    quo, rem = total // one, total % one
    return np.where(cnt > 0, quo + (np.uint64(2) * rem >= one).astype(np.uint64), c)


def kmeans_centres(c: np.ndarray, mn, step, T) -> np.ndarray:
    """``q``: the centres back in the data's type, ``(K, 1)``."""
    return (mn + c.astype(np.float64) * step).astype(T).reshape(-1, 1)


class QuantizedKmeans(QuantizedCompressor):
    """The reference's ``QuantizedKmeans`` (arXiv:1510.00149) with a pinned
    fit: integer Lloyd steps from a deterministic start; the module's
    docstring has the definition.  ``init`` is ``"cbrt"`` or an array of
    ``n_clusters`` non-decreasing centres; ``None``, the reference's random
    start, is refused."""

    KmeansCompressData = KmeansCompressData

    def __init__(self, quant_bits: int = 8, n_clusters=None, init=None, max_iter: int = 50):
        super().__init__(quant_bits)
        self.n_clusters = K = int(quant_bits if n_clusters is None else n_clusters)
        if K < 2 or K > (1 << quant_bits):
            raise ValueError(f"QuantizedKmeans: n_clusters must be in 2..2^quant_bits = {1 << quant_bits}, got {K}: "
                             "a label beyond 2^quant_bits has no code")
        if init is None:
            raise ValueError("QuantizedKmeans: init=None, scikit-learn's random start, is not built; pass "
                             "init='cbrt' or an array of n_clusters sorted centres")
        if isinstance(init, str):
            if init != "cbrt":
                raise ValueError(f"QuantizedKmeans: init is 'cbrt' or an array of centres, not {init!r}")
        else:
            init = np.asarray(_host(init) if isinstance(init, torch.Tensor) else init).reshape(-1)
            if init.size != K or init.dtype.kind != "f" or not np.all(init[1:] >= init[:-1]):
                raise ValueError(f"QuantizedKmeans: init as an array is {K} non-decreasing floating-point centres")
        if int(max_iter) < 1:
            raise ValueError(f"QuantizedKmeans: max_iter must be at least 1, got {max_iter}")
        self.init, self.max_iter = init, int(max_iter)

    def _start(self, hist, mn, s) -> np.ndarray:
        """The first centres as uint64; ``hist`` gives the histogram when the start needs it."""
        if isinstance(self.init, str):
            return kmeans_init(hist(), self.n_clusters)
        return kmeans_image(self.init, mn, s)

    def _compress_one(self, data, name="[0]"):
        K, bits = self.n_clusters, self.quant_bits
        w = _Where(data, name, "QuantizedKmeans")
        self._device_bits(w, name)
        n = w.flat.numel() if w.device is not None else w.flat.size
        if n == 0:
            raise _refuse(name, "no element at all")
        if n <= K:
            return KmeansCompressData(data, bits)  # as the reference: too few elements to cluster
        if n >> 32:
            raise ValueError(f"QuantizedKmeans: entry {name} has 2^32 elements or more")
        if w.device is not None and K > KMEANS_DEVICE_MAX_K:
            raise ValueError(f"QuantizedKmeans: entry {name} is a device tensor, which takes n_clusters <= "
                             f"{KMEANS_DEVICE_MAX_K} (got {K}); host arrays take any")
        mn, mx, _ = w.range()
        mn, s, step = kmeans_scale(mn, mx, name)
        fit = self._fit_device if w.device is not None else self._fit_host
        codes, c, n_iter = fit(w, mn, s)
        return KmeansCompressData(codes, bits, w.dtype, kmeans_centres(c, mn, step, w.dtype.type), n_iter)

    def _fit_host(self, w: _Where, mn, s):
        K, half = self.n_clusters, 1 << (self.quant_bits - 1)
        u = kmeans_image(w.flat, mn, s)
        c = self._start(lambda: np.bincount((u >> np.uint64(KMEANS_BIN_SHIFT)).astype(np.int64),
                                            minlength=KMEANS_BINS), mn, s)
        lo, hi = (u & np.uint64(0xFFFF)).astype(np.float64), (u >> np.uint64(16)).astype(np.float64)
        n_iter = 0
        while n_iter < self.max_iter:
            label = np.searchsorted((c[:-1] + c[1:]) >> np.uint64(1), u, side="left")
            cnt = np.bincount(label, minlength=K).astype(np.uint64)
            # the sums in two 16-bit halves: each half's float64 sum stays below 2^48, so it is exact
            total = (np.bincount(label, weights=hi, minlength=K).astype(np.uint64) << np.uint64(16)) \
                + np.bincount(label, weights=lo, minlength=K).astype(np.uint64)
            new = kmeans_update(c, cnt, total)
            n_iter += 1
            same = np.array_equal(new, c)
            c = new
            if same:
                break
        label = np.searchsorted((c[:-1] + c[1:]) >> np.uint64(1), u, side="left")
        return w.wrap((label - half).astype(self.np_type)), c, n_iter

    def _fit_device(self, w: _Where, mn, s):
        from .. import _lib as L
        from .. import hostpipe as H
        from .. import kernels as Kn
        from .compressor import _scratch_for

        K, x = self.n_clusters, w.flat
        scratch = _scratch_for(x, Kn.kmeans_scratch_bytes(x.numel(), x.dtype))  # the histogram, then the state
        hist = scratch[:4 * KMEANS_BINS].view(torch.int32)
        state = scratch[4 * KMEANS_BINS:4 * KMEANS_BINS + L.SA_KMEANS_STATE_BYTES]
        c0 = self._start(lambda: H.d2h(Kn.kmeans_hist(x, mn, s, hist), pooled=False).view(np.uint32), mn, s)
        words = np.zeros(L.SA_KMEANS_STATE_BYTES // 4, dtype=np.uint32)
        words[L.SA_KMEANS_STATE_C // 4:][:K] = c0
        state.copy_(H.h2d(words.view(np.uint8), x.device))
        Kn.kmeans_step(x, mn, s, K, self.max_iter, state)
        codes = Kn.kmeans_labels(x, mn, s, K, state, 1 << (self.quant_bits - 1), w.codes(self.np_type))
        tail = H.d2h(state[L.SA_KMEANS_STATE_C:].view(torch.int32), pooled=False).view(np.uint32)
        n_iter = int(tail[(L.SA_KMEANS_STATE_DONE - L.SA_KMEANS_STATE_C) // 4 + 1])
        return codes.reshape(w.shape), tail[:K].astype(np.uint64), n_iter

    def _decompress_one(self, c, name="[0]"):
        if c.q is None:  # passed through
            return c.compressed_data
        codes, on_device, was_tensor = _codes_of(c, _store_type(c.quant_bits), name, "QuantizedKmeans")
        T, half = c.origin_type.type, 1 << (c.quant_bits - 1)
        q = np.ascontiguousarray(np.asarray(c.q).reshape(-1), dtype=T)
        K = q.size
        if on_device:
            from .. import hostpipe as H
            from .. import kernels as Kn

            out = torch.empty(codes.numel(), dtype=_torch_dtype(c.origin_type), device=codes.device)
            bad, at = 0, 0
            if codes.numel():
                flag = Kn.coo_flag(codes.device)
                Kn.dequant_lut(codes, H.h2d(q, codes.device), half, out, flag)
                bad, at = (int(v) for v in H.d2h(flag, pooled=False).view(np.uint32))
            dec = out
        else:
            label = codes.astype(np.int64) + half
            wrong = (label < 0) | (label >= K)
            bad, at = bool(wrong.any()), int(np.argmax(wrong))
            dec = None if bad else q[label]
        if bad:
            raise ValueError(f"QuantizedKmeans: entry {name} holds a code outside the {K} clusters at position {at}")
        return _unwrap(dec, tuple(c.compressed_data.shape), was_tensor)
