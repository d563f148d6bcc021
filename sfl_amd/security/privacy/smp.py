"""FedSMP, sparsified model perturbation: the worker's step and the mask it
shares with the server.

Mirrors ``examples/security/h_gia/FedSMP_defense/FedSMP_torch.py:105-119``
(the worker) and ``:193-201`` (the server's mask).  The reference's worker
takes its update ``new - old``, multiplies it by a random 0/1 mask, divides
by ``compression_ratio + 1e-6``, runs ``GaussianModelDP`` on the result,
multiplies by the mask again and uploads ``old +`` that.

Definition (include/sfl_sa.h carries the same text for the kernels):

**Mask.**  ``SMPMask(key: uint64, ratio p in [0, 1])``.  The threshold is
``T = min(2**32, int(p * 4294967296))`` in Python integer arithmetic (the
product is exact in a double).  The elements of the payload's float32
entries take consecutive stream indices ``i = counter0 + e``, ``counter0``
the sum of ``ceil(n / 4) * 4`` over the float32 entries before (the layout
of ``GaussianModelDP.counter``).  ``w_i`` is word ``i & 3`` of Philox4x32-10
on the counter block ``(lo32(i >> 2), hi32(i >> 2), 1, 0)`` under the key
words ``(lo32(key), hi32(key))``; the ``1`` keeps the mask's words apart
from the DP noise's, which has ``0`` there, so a mask and a noise stream
under one key are still independent.  An element is kept iff ``w_i < T``,
compared in 64 bits: ``p = 1`` keeps everything, ``p = 0`` nothing.  Entries
that are not float32 (``num_batches_tracked``) take no indices, are not part
of the norm and upload their trained value unchanged.

**Worker arithmetic**, float32, every operation rounded separately:
``c = np.float32(p + 1e-6)`` (the double sum, rounded once); ``g = w1 - w0``;
``d = kept ? g / c : +0`` (an IEEE division); the layers' squared norms,
the clip scale and ``t = d * scale + (z * sigma) / num_updates`` are
``GaussianModelDP``'s own on the list of ``d`` (noise index ``counter + e``:
the normals of dropped elements are skipped, never reused);
``out = kept ? w0 + t : w0``; without a ``model_gdp``, ``t = d``.

**Refinements over the reference.**

1. float32 throughout.  The reference's mask is an int64 array, which
   promotes the update, the norm and the upload to float64 by accident; here
   the payload keeps the model's float32, as every other strategy's does.
2. A select instead of ``0 * x``: a dropped element is ``w0`` exactly.  The
   reference turns ``0 * inf`` into NaN and can flip the sign of a zero.
3. A keyed stream instead of a shipped mask.  The reference draws
   ``np.random.binomial`` from numpy's unseeded global stream and sends the
   array (8 bytes per parameter) to every party every round; parity for the
   mask is therefore distributional, as for the DP noise.  Here the server
   sends ``(key, p)``, 16 bytes, and every party regenerates the mask inside
   the kernel that uses it.
4. Integer entries pass through; the reference multiplies them by the mask.

``smp_step`` has three forms that give the same bits from the same keys and
counters:

* host arrays: the mask from ``sa_smp_mask_host``, numpy in float32,
  ``model_gdp(list)`` if one is given, the numpy finish;
* CUDA tensors, fused: with a Philox ``GaussianModelDP`` on the tensors'
  device (or none), two streaming passes per layer that materialise neither
  the update nor the mask: ``sa_smp_sumsq_f32`` (reads ``old`` and ``new``)
  and ``sa_smp_perturb_f32`` (reads both, writes the upload);
* CUDA tensors, unfused: with any other ``model_gdp``
  (``SecureGaussianModelDP``, a callable of the user's),
  ``sa_smp_delta_f32``, then ``model_gdp``, then ``sa_smp_finish_f32``.
"""

from __future__ import annotations

import hashlib
import secrets
from typing import List, Optional

import numpy as np
import torch

from ... import _lib as L
from ... import hostpipe as H
from ... import kernels as K
from .mechanism import GaussianModelDP

_M64 = (1 << 64) - 1


class SMPMask:
    """One round's mask: what the server sends in place of the reference's
    int64 arrays.  ``key`` is 64 bits, ``ratio`` the keep probability."""

    nbytes = 16  # on the wire: the key and the ratio, 8 bytes each

    def __init__(self, key: int, ratio: float):
        ratio = float(ratio)
        if not 0.0 <= ratio <= 1.0:
            raise ValueError(f"ratio should be between 0 and 1, but got {ratio}")
        self.key = int(key) & _M64
        self.ratio = ratio

    @property
    def threshold(self) -> int:
        return min(1 << 32, int(self.ratio * 4294967296))

    @property
    def divisor(self) -> np.float32:
        return np.float32(self.ratio + 1e-6)

    def layer(self, counter0: int) -> L.SMP:
        """The sa_smp of a layer whose first element has stream index ``counter0``."""
        return K.make_smp(self.key, counter0, self.threshold, float(self.divisor))

    def kept(self, counter0: int, n: int) -> np.ndarray:
        """The mask of ``n`` elements from stream index ``counter0`` as a host bool array."""
        return L.smp_mask_host(self.layer(counter0), n).astype(bool)

    def __eq__(self, other):
        return isinstance(other, SMPMask) and (other.key, other.ratio) == (self.key, self.ratio)

    def __hash__(self):
        return hash(("SMPMask", self.key, self.ratio))

    def __repr__(self):
        return f"SMPMask(key={self.key:#018x}, ratio={self.ratio})"


def mask_key(random_seed: Optional[int], draw: int) -> int:
    """The server's key of mask ``draw`` (0: with the initial average, then
    one per aggregation).  Without a seed, 64 bits from the OS CSPRNG; with
    one, the first 8 bytes (little-endian) of
    ``SHA-256(b"sfl_amd.fed_smp.mask" + seed + draw)``, seed and draw as
    8-byte little-endian words (the seed modulo 2^64), so that a test can
    follow the sequence."""
    if random_seed is None:
        return secrets.randbits(64)
    h = hashlib.sha256(b"sfl_amd.fed_smp.mask" + (int(random_seed) & _M64).to_bytes(8, "little")
                       + int(draw).to_bytes(8, "little")).digest()
    return int.from_bytes(h[:8], "little")


def _is_f32(a) -> bool:
    dt = a.dtype
    if dt in (torch.float32, np.float32):
        return True
    floating = dt.is_floating_point if isinstance(dt, torch.dtype) else np.issubdtype(dt, np.floating)
    if floating:
        raise NotImplementedError(f"fed_smp: float32 models only, not {dt}")
    return False


def _flat(a: torch.Tensor) -> torch.Tensor:
    """The layer as a flat 16-byte aligned tensor (a misaligned view is copied, as GaussianModelDP._flat does)."""
    t = a.detach().reshape(-1).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _counters(sizes) -> List[int]:
    out, c = [], 0
    for n in sizes:
        out.append(c)
        c += -(-n // 4) * 4
    return out


def _step_host(old, new, mask: SMPMask, model_gdp):
    c = mask.divisor
    olds = [np.asarray(a, dtype=np.float32) for a in old]
    kept = [mask.kept(c0, a.size).reshape(a.shape) for a, c0 in zip(olds, _counters([a.size for a in olds]))]
    with np.errstate(all="ignore"):  # an inf or a NaN in a weight is the caller's to see, not numpy's to warn of
        ds = [np.where(k, (np.asarray(n, dtype=np.float32) - o) / c, np.float32(0)) for o, n, k in zip(olds, new, kept)]
        ts = [np.asarray(t, dtype=np.float32) for t in model_gdp(ds)] if model_gdp is not None and ds else ds
        return [np.where(k, o + t.reshape(o.shape), o) for o, t, k in zip(olds, ts, kept)]


def _step_device(old, new, mask: SMPMask, model_gdp):
    dev = old[0].device
    shapes = [tuple(a.shape) for a in old]
    w0s, w1s = [_flat(a) for a in old], [_flat(a) for a in new]
    smps = [mask.layer(c0) for c0 in _counters([w.numel() for w in w0s])]
    fused = model_gdp is None or (type(model_gdp) is GaussianModelDP and model_gdp.device == dev)
    if not fused:
        ds = [K.smp_delta(w0, w1, s, torch.empty_like(w0)) if w0.numel() else torch.empty_like(w0)
              for w0, w1, s in zip(w0s, w1s, smps)]
        ts = [t if isinstance(t, torch.Tensor) else H.h2d(np.asarray(t, dtype=np.float32), dev) for t in model_gdp(ds)]
        ts = [_flat(t.to(device=dev, dtype=torch.float32)) for t in ts]
        return [(K.smp_finish(w0, t, s, torch.empty_like(w0)) if w0.numel() else torch.empty_like(w0)).reshape(shape)
                for w0, t, s, shape in zip(w0s, ts, smps, shapes)]
    if model_gdp is None:
        return [(K.smp_perturb(w0, w1, s, None, torch.empty_like(w0)) if w0.numel() else torch.empty_like(w0))
                .reshape(shape) for w0, w1, s, shape in zip(w0s, w1s, smps, shapes)]
    part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    for w0, w1, s in zip(w0s, w1s, smps):  # GaussianModelDP.sumsq over d, d never stored
        if w0.numel():
            K.smp_sumsq(w0, w1, s, total, part, accumulate=True)
    out = []
    for w0, w1, s, shape in zip(w0s, w1s, smps, shapes):
        layer = None
        if model_gdp.is_clip_each_layer:
            layer = torch.zeros(1, dtype=torch.float64, device=dev)
            if w0.numel():
                K.smp_sumsq(w0, w1, s, layer, part)
        dp = model_gdp.params(total, w0.numel(), layer)  # advances the noise counter as __call__ would
        y = torch.empty_like(w0)
        if w0.numel():
            K.smp_perturb(w0, w1, s, dp, y)
        out.append(y.reshape(shape))
    return out


def smp_step(old: list, new: list, mask: SMPMask, model_gdp=None) -> list:
    """A worker's upload for the round's weights ``old``, its trained weights
    ``new`` (lists of layers: all host arrays, or all tensors of one GPU) and
    the server's ``mask``.  float32 entries come back as float32 where they
    lived; other entries are ``new``'s, untouched."""
    if len(old) != len(new):
        raise ValueError("smp_step: old and new differ in length")
    idx = [i for i, a in enumerate(old) if _is_f32(a)]
    out = list(new)
    if not idx:
        return out
    o, n = [old[i] for i in idx], [new[i] for i in idx]
    cuda = [isinstance(a, torch.Tensor) and a.is_cuda for a in (*o, *n)]
    if all(cuda):
        res = _step_device(o, n, mask, model_gdp)
    elif not any(cuda):
        host = [a.detach().numpy() if isinstance(a, torch.Tensor) else a for a in (*o, *n)]
        res = _step_host(host[:len(o)], host[len(o):], mask, model_gdp)
    else:
        raise ValueError("smp_step: the float32 layers are all host arrays or all tensors of one GPU")
    for i, r in zip(idx, res):
        out[i] = r
    return out
