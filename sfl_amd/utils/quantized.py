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
