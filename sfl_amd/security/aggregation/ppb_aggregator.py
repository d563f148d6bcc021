"""The batched Paillier aggregator, mirroring the reference's ``PPBAggregator``
("phe_paillier_batch_aggregator",
``sfl/security/aggregation/experiment/ppb_aggregator.py:249-420``): the
additively homomorphic alternative to masking.  Every party packs several
fixed-point fields into one Paillier plaintext and encrypts; the server
multiplies the parties' ciphertexts modulo ``n^2``, decrypts once and unpacks.

The definition (``C`` parties, key size ``K`` bits, ``len`` =
``len_after_encode``, ``bias``, ``expand``; ``ppb_host`` below is the same text
in Python integers, and the device path computes the same numbers with the
``sa_ppb_*`` entries of include/sfl_sa.h):

1. **Fields.**  ``per_row = K // len`` fields go into one plaintext (``:45-47``;
   37 at 2048 bits).  The elements of a layer, flattened, are cut into rows of
   ``per_row``; the last row may hold fewer (the reference's
   ``size_of_per_col``).  The first element of a row is its most significant
   field: ``plaintext = sum_i field_i << (len * (cnt - 1 - i))`` for the row's
   ``cnt`` fields (``:111-113``).
2. **Field value.**  ``int(abs(x * w / total + bias) * expand)`` (``:74-75`` and
   ``:105``), every step a float64 operation in this order, the element
   converted to float64 first.  ``sum`` is ``w = total = 1``.  ``average``
   pre-scales each party with its weight over the weights' total and divides by
   nothing after decoding; that this happens in float64 for float32 uploads is
   a refinement (the reference's result type there depends on the numpy
   version).  Per-element weights are multiplied in float64 beforehand
   (``x * w / total`` as array operations) and the fields are then taken with
   ``w = total = 1``.
   Every field must satisfy ``x * w / total + bias >= 0``, not NaN, and
   ``field * C < 2^len`` so that the sum of ``C`` parties cannot carry into
   the neighbouring field; otherwise ``OverflowError`` names the party (the
   reference corrupts the neighbouring field silently).
3. **Paillier** with ``g = n + 1``.  Encrypt: ``c = (1 + m n) r^n mod n^2``.
   Add: the product of the parties' ciphertexts mod ``n^2`` (``:169-185``).
   Decrypt: ``m = ((c^lambda mod n^2 - 1) / n) mu mod n`` with ``lambda =
   lcm(p - 1, q - 1)`` and ``mu = ((g^lambda mod n^2 - 1) / n)^-1 mod n``.
   Keys are made on the host in Python integers (``secrets``, Miller-Rabin
   with 40 random bases): ``p`` and ``q`` of ``K / 2`` bits each with their top
   two bits set, so ``n`` has exactly ``K`` bits.  ``K`` is a multiple of 64,
   at least 128, and ``per_row * len < K`` (a plaintext is below ``n``).
4. **The randomness.**  Each party holds a 32-byte ChaCha20 key
   (``secrets.token_bytes``); the nonce is the party's call counter, so a
   ``(key, nonce, block)`` triple is never used twice.  Ciphertexts of one
   call are numbered ``j`` through all its layers in order.  Candidate ``t`` of
   ciphertext ``j`` is the first ``K / 32`` words of the keystream as
   little-endian limbs, starting at block ``(64 j + t) ceil(K / 512)``; ``r_j``
   is the first candidate with ``0 < r < n`` for ``t < 64``.  If none
   qualifies (probability at most ``2^-64``) ``RuntimeError`` is raised.
   ``gcd(r, n) != 1`` would reveal a factor of ``n``, has negligible
   probability and is not tested for.
5. **Decode.**  ``field / expand - C * bias`` (``:219-221``) in float64: the
   correctly rounded conversion of the integer, the IEEE division, the
   subtraction.  Results are float64 in the uploads' shapes -- numpy arrays for
   host uploads, tensors that stay on the device for CUDA uploads; casting them
   to float32 gives the values of the reference's ``torch.tensor(...)``.

When any layer of the uploads is a CUDA tensor, the whole call runs on that
device; the host form serves host uploads and every case the kernels refuse (a
key size other than 128, 256, 512, 1024, 2048, a field width outside 32..63),
counted in ``last_report["host_fallback"]``.  The two forms share everything
except the big-number arithmetic: they give the same ciphertexts from the same
randomness, and the same results.

The class is experimental in the reference ("for experiment purpose only"),
and so is this: the server holds the private key and sees every party's
ciphertext, and the kernels are not constant-time against a co-tenant of the
device.
"""

from __future__ import annotations

import math
import secrets
from typing import List, Sequence

import numpy as np
import torch

from ...device import PYU, DeviceObject
from .aggregator import Aggregator

FLAG_NEGATIVE, FLAG_NAN, FLAG_RANGE, FLAG_NO_R = 1, 2, 4, 8  # SA_PPB_FLAG_*
CANDIDATES = 64
_SMALL_PRIMES = [p for p in range(3, 2000, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]


# -------------------------------------------------------------------- the key
def is_prime(v: int, rounds: int = 40) -> bool:
    """Miller-Rabin with random bases."""
    if v < 2 or v % 2 == 0:
        return v == 2
    for p in _SMALL_PRIMES:
        if v % p == 0:
            return v == p
    d, s = v - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(rounds):
        x = pow(2 + secrets.randbelow(v - 3), d, v)
        if x in (1, v - 1):
            continue
        for _ in range(s - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def random_prime(bits: int) -> int:
    """A prime of ``bits`` bits with its top two bits set."""
    while True:
        v = secrets.randbits(bits) | (3 << (bits - 2)) | 1
        if is_prime(v):
            return v


def limbs(v: int, count: int) -> np.ndarray:
    """``v`` as ``count`` little-endian uint32 limbs."""
    return np.frombuffer(int(v).to_bytes(4 * count, "little"), dtype=np.uint32).copy()


def from_limbs(a) -> int:
    return int.from_bytes(np.ascontiguousarray(a, dtype=np.uint32).tobytes(), "little")


class PaillierKey:
    """``n`` and, for the server, ``lambda`` and ``mu``."""

    def __init__(self, p: int, q: int):
        if p == q or not (is_prime(p) and is_prime(q)) or p.bit_length() != q.bit_length():
            raise ValueError("p and q are two different primes of one size")
        self.n = p * q
        self.bits = 2 * p.bit_length()
        if self.n.bit_length() != self.bits or self.bits % 64 or self.bits < 128:
            raise ValueError(f"n = p q must have exactly {self.bits} bits, a multiple of 64 and at least 128")
        self.n2 = self.n * self.n
        self.lam = math.lcm(p - 1, q - 1)
        self.mu = pow((pow(self.n + 1, self.lam, self.n2) - 1) // self.n, -1, self.n)

    @classmethod
    def generate(cls, bits: int) -> "PaillierKey":
        if bits % 64 or bits < 128:
            raise ValueError(f"paillier_key_size is a multiple of 64 and at least 128, not {bits}")
        while True:
            p, q = random_prime(bits // 2), random_prime(bits // 2)
            if p != q:
                key = cls(p, q)
                key.p, key.q = p, q
                return key

    def encrypt(self, m: int, r: int) -> int:
        return (1 + m * self.n) * pow(r, self.n, self.n2) % self.n2

    def decrypt(self, c: int) -> int:
        return (pow(c, self.lam, self.n2) - 1) // self.n * self.mu % self.n

    def consts(self, private: bool = True) -> np.ndarray:
        """The constants buffer of the ``sa_ppb_*`` entries (include/sfl_sa.h)."""
        ln, mask = self.bits // 32, (1 << 32) - 1
        R, Rn = 1 << (2 * self.bits), 1 << self.bits
        head = [self.bits, -pow(self.n2, -1, 1 << 32) & mask, -pow(self.n, -1, 1 << 32) & mask,
                self.lam.bit_length() if private else 0, 0, 0, 0, 0]
        return np.concatenate([np.array(head, dtype=np.uint32), limbs(self.n2, 2 * ln), limbs(R * R % self.n2, 2 * ln),
                               limbs(R % self.n2, 2 * ln), limbs(self.n * R % self.n2, 2 * ln), limbs(self.n, ln),
                               limbs(self.lam if private else 0, ln),
                               limbs(self.mu * Rn % self.n if private else 0, ln)])


def draw_r(key: bytes, nonce: int, j: int, n: int, bits: int) -> int:
    """Step 4 for ciphertext ``j``; None when no candidate qualifies."""
    from ... import _lib as L

    blocks = -(-bits // 512)
    for t in range(CANDIDATES):
        words = L.chacha20_blocks_host(key, nonce, (CANDIDATES * j + t) * blocks, blocks).reshape(-1)[:bits // 32]
        r = from_limbs(words)
        if 0 < r < n:
            return r
    return None


# ----------------------------------------------------------------- the fields
def fields_host(x: np.ndarray, w: float, total: float, bias: float, expand: float, bits: int, parties: int) -> tuple:
    """Step 2 for one flattened layer: (the fields as Python integers, the flag word)."""
    with np.errstate(all="ignore"):
        s = np.asarray(x).reshape(-1).astype(np.float64) * np.float64(w) / np.float64(total) + np.float64(bias)
        p = np.abs(s) * np.float64(expand)
    nan, neg = np.isnan(s), s < 0
    limit = ((1 << bits) - 1) // parties
    ok = ~nan & ~neg & (p < float(1 << bits))
    out = [int(v) if good else 0 for v, good in zip(p.tolist(), ok.tolist())]
    big = [good and v > limit for v, good in zip(out, ok.tolist())]
    flags = (FLAG_NAN if nan.any() else 0) | (FLAG_NEGATIVE if (neg & ~nan).any() else 0) \
        | (FLAG_RANGE if (~nan & ~neg & ~ok).any() or any(big) else 0)
    return [0 if b else v for v, b in zip(out, big)], flags


def pack_host(fields: Sequence[int], per_row: int, bits: int) -> List[int]:
    """Step 1: the plaintexts of one layer's fields."""
    rows = []
    for at in range(0, len(fields), per_row):
        m = 0
        for f in fields[at:at + per_row]:
            m = (m << bits) | f
        rows.append(m)
    return rows


def unpack_host(rows: Sequence[int], count: int, per_row: int, bits: int) -> List[int]:
    out = []
    for i, m in enumerate(rows):
        cnt = min(per_row, count - i * per_row)
        out += [(m >> (bits * (cnt - 1 - k))) & ((1 << bits) - 1) for k in range(cnt)]
    return out


def decode_host(fields: Sequence[int], expand: float, bias: float, parties: int) -> np.ndarray:
    """Step 5."""
    return np.array([float(f) for f in fields], np.float64) / np.float64(expand) - np.float64(parties * bias)


def _refuse(flags: int, party: int) -> None:
    if flags & (FLAG_NEGATIVE | FLAG_NAN | FLAG_RANGE):
        why = [s for b, s in ((FLAG_NEGATIVE, "x + bias is negative"), (FLAG_NAN, "a NaN"),
                              (FLAG_RANGE, "a field too large for the parties' sum to stay in its bits")) if flags & b]
        raise OverflowError(f"party {party}: {', '.join(why)}: the value cannot be packed (bias_of_weight, "
                            f"expand_of_weight and len_after_encode bound what can)")
    if flags & FLAG_NO_R:
        raise RuntimeError(f"party {party}: no r below n among {CANDIDATES} candidates")


class PPBAggregator(Aggregator):
    """phe_paillier_batch_aggregator: experimental, as in the reference.

    ``sum`` and ``average`` over the parties run the module's definition on
    single arrays or lists of layers and give float64 results in the uploads'
    shapes (cast to float32 for the reference's values).  CUDA uploads are
    encoded, encrypted, added, decrypted and decoded on their device and the
    results stay there; ``last_report`` holds ``host_fallback`` (1 when CUDA
    uploads had to take the host form), ``rows`` and ``key_bits``.

    Examples:
      >>> aggregator = PPBAggregator(server, [alice, bob])
      >>> fl = FLModel(server=server, device_list=[alice, bob], model=build, aggregator=aggregator)
    """

    def __init__(self, device: PYU, participants: List[PYU], paillier_key_size=2048, len_after_encode=55,
                 bias_of_weight=20, expand_of_weight=10e12, *, _primes=None, _party_keys=None):
        assert isinstance(device, PYU), f"Accepts PYU only but got {type(device)}."
        self.device = device
        self.parties = len(participants)
        self.key = PaillierKey(*_primes) if _primes else PaillierKey.generate(int(paillier_key_size))
        self.bits = self.key.bits
        self.len, self.bias, self.expand = int(len_after_encode), float(bias_of_weight), float(expand_of_weight)
        self.per_row = self.bits // self.len
        if not 1 <= self.len <= 63 or self.per_row < 1 or self.per_row * self.len >= self.bits or self.parties < 1:
            raise ValueError("len_after_encode is in 1..63 with per_row * len_after_encode below the key size, and "
                             "there is at least one participant")
        self.party_keys = list(_party_keys) if _party_keys else [secrets.token_bytes(32) for _ in range(self.parties)]
        if len(self.party_keys) != self.parties:
            raise ValueError("one ChaCha20 key per participant")
        self.calls = 0  # the parties' call counter: the ChaCha20 nonce
        self.last_report = None
        self._consts = {}

    @classmethod
    def from_primes(cls, device: PYU, participants: List[PYU], p: int, q: int, **kw) -> "PPBAggregator":
        """An aggregator over the key ``n = p q`` (tests; a deployment's key never leaves the server)."""
        return cls(device, participants, _primes=(p, q), **kw)

    # ------------------------------------------------------------ the paths
    def _host(self, layers: list, scale: list) -> list:
        """``layers[l][i]`` numpy arrays, ``scale[i] = (w, total)``: the host form."""
        k, nonce = self.key, self.calls
        sums, j0 = [], 0
        for xs in layers:
            rows = None
            for i, x in enumerate(xs):
                f, flags = fields_host(x, *scale[i], self.bias, self.expand, self.len, self.parties)
                _refuse(flags, i)
                plain = pack_host(f, self.per_row, self.len)
                cts = []
                for j, m in enumerate(plain):
                    r = draw_r(self.party_keys[i], nonce, j0 + j, k.n, self.bits)
                    if r is None:
                        _refuse(FLAG_NO_R, i)
                    cts.append(k.encrypt(m, r))
                rows = cts if rows is None else [a * b % k.n2 for a, b in zip(rows, cts)]
            j0 += len(rows)
            sums.append([k.decrypt(c) for c in rows])
        return [decode_host(unpack_host(rows, xs[0].size, self.per_row, self.len), self.expand, self.bias,
                            self.parties).reshape(xs[0].shape) for rows, xs in zip(sums, layers)]

    def _device_consts(self, dev, private: bool) -> torch.Tensor:
        from ... import hostpipe as H

        if (dev, private) not in self._consts:
            self._consts[dev, private] = H.h2d(self.key.consts(private).view(np.int32), dev)
        return self._consts[dev, private]

    def _device(self, layers: list, scale: list, dev) -> list:
        """``layers[l][i]`` flat tensors on ``dev``: the device form."""
        from ... import hostpipe as H
        from ... import kernels as K

        ln = self.bits // 32
        counts = [xs[0].numel() for xs in layers]
        starts = np.concatenate([[0], np.cumsum([-(-n // self.per_row) for n in counts])]).astype(int)
        rows = int(starts[-1])
        public, private = self._device_consts(dev, False), self._device_consts(dev, True)
        flags = torch.zeros(self.parties, dtype=K.LIMB, device=dev)
        cts = []
        for i in range(self.parties):
            plain = torch.empty(rows * ln, dtype=K.LIMB, device=dev)
            for l, xs in enumerate(layers):
                if counts[l]:
                    K.ppb_encode(xs[i], *scale[i], self.parties, self.bias, self.expand, self.bits, self.len,
                                 plain[int(starts[l]) * ln:], flags[i:i + 1])
            ct = torch.empty(2 * rows * ln, dtype=K.LIMB, device=dev)
            if rows:
                K.ppb_encrypt(plain, rows, self.bits, public, self.party_keys[i], self.calls, ct, flags[i:i + 1])
            cts.append(ct)
        total = torch.empty(2 * rows * ln, dtype=K.LIMB, device=dev)
        plain = torch.empty(rows * ln, dtype=K.LIMB, device=dev)
        if rows:
            K.ppb_add(cts, rows, self.bits, public, total)
            K.ppb_decrypt(total, rows, self.bits, private, cts[0], plain)
        outs = []
        for l, xs in enumerate(layers):
            out = torch.empty(counts[l], dtype=torch.float64, device=dev)
            if counts[l]:
                K.ppb_decode(plain[int(starts[l]) * ln:], self.parties, self.bias, self.expand, self.bits, self.len, out)
            outs.append(out.reshape(tuple(xs[0].shape)))
        for i, word in enumerate(H.d2h(flags, pooled=False)):  # the one read of the refusals
            _refuse(int(word), i)
        return outs

    def _aggregate(self, parties: list, weights):
        from ... import _lib as L
        from ... import hostpipe as H

        if len(parties) != self.parties:
            raise ValueError(f"{len(parties)} uploads for {self.parties} participants")
        single = not isinstance(parties[0], (list, tuple))
        data = [[p] if single else list(p) for p in parties]
        data = [[x if isinstance(x, torch.Tensor) else np.asarray(x) for x in d] for d in data]
        if any(len(d) != len(data[0]) for d in data):
            raise ValueError("every party uploads the same number of layers")
        layers = [[d[l] for d in data] for l in range(len(data[0]))]
        for l, xs in enumerate(layers):
            if any(tuple(x.shape) != tuple(xs[0].shape) for x in xs):
                raise ValueError(f"layer {l}: the parties' shapes differ")
        dev = next((x.device for xs in layers for x in xs if isinstance(x, torch.Tensor) and x.is_cuda), None)
        # weights: scalars go into the encoding; arrays are multiplied in float64 first
        scale = [(1.0, 1.0)] * self.parties
        if weights is not None:
            ws = [w if isinstance(w, torch.Tensor) else np.asarray(w) for w in weights]
            if len(ws) != self.parties:
                raise ValueError(f"weights: one per participant ({self.parties}) or None")
            if all(w.ndim == 0 for w in ws):
                ws = [float(w) for w in ws]
                scale = [(w, float(sum(ws))) for w in ws]
            else:
                f64 = (lambda v: torch.as_tensor(v).to(dev, torch.float64)) if dev is not None else \
                    (lambda v: np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, np.float64))
                ws = [f64(w) for w in ws]
                total = ws[0]
                for w in ws[1:]:
                    total = total + w
                layers = [[f64(x) * ws[i] / total for i, x in enumerate(xs)] for xs in layers]
        report = {"host_fallback": 0, "key_bits": self.bits,
                  "rows": sum(-(-int(np.prod(xs[0].shape)) // self.per_row) for xs in layers)}
        if dev is not None and (self.bits not in L.SA_PPB_KEY_BITS or not 32 <= self.len <= 63
                                or any(x.dtype not in (torch.float32, torch.float64, torch.int64)
                                       for xs in layers for x in xs if isinstance(x, torch.Tensor))):
            report["host_fallback"] = 1
        if dev is not None and not report["host_fallback"]:
            flat = [[(x.detach() if isinstance(x, torch.Tensor) and x.is_cuda else H.h2d(x, dev)).contiguous()
                     .reshape(-1) for x in xs] for xs in layers]
            for row, xs in zip(flat, layers):
                if any(x.dtype != row[0].dtype for x in row):
                    raise ValueError("a layer has one element type in every party")
            outs = [o.reshape(tuple(xs[0].shape)) for o, xs in zip(self._device(flat, scale, dev), layers)]
        else:
            host = [[H.d2h(x, pooled=False) if isinstance(x, torch.Tensor) and x.is_cuda else
                     (x.detach().numpy() if isinstance(x, torch.Tensor) else x) for x in xs] for xs in layers]
            outs = self._host(host, scale)
            if dev is not None:
                outs = [H.h2d(o, dev) for o in outs]
        self.calls += 1
        self.last_report = report
        return outs[0] if single else outs

    # --------------------------------------------------------------- surface
    def _run(self, data: List[DeviceObject], fn):
        assert data, "Data to aggregate should not be None or empty!"
        data = [d.to(self.device) for d in data]
        return self.device(fn)(*data)

    def sum(self, data: List[DeviceObject], axis=None) -> DeviceObject:
        """Sum over the parties of the encrypted uploads."""
        if axis not in (None, 0):
            raise ValueError(f"PPBAggregator aggregates over the parties (axis 0 or None), not axis {axis}")
        return self._run(data, lambda *parties: self._aggregate(list(parties), None))

    def average(self, data: List[DeviceObject], axis=None, weights=None) -> DeviceObject:
        """Weighted average over the parties of the encrypted uploads."""
        if axis not in (None, 0):
            raise ValueError(f"PPBAggregator aggregates over the parties (axis 0 or None), not axis {axis}")
        if weights is None:
            weights = [1.0] * self.parties
        weights = [wt.to(self.device).data if isinstance(wt, DeviceObject) else wt for wt in weights]
        return self._run(data, lambda *parties: self._aggregate(list(parties), weights))
