"""SecureAggregator on MI355X: the drop-in for
``secretflow.security.aggregation.SecureAggregator`` (un-vendored,
``secretflow-lite==1.13.0b0``; constructor ``(device, participants,
fxp_bits=18)`` as subclassed at
``sfl/security/aggregation/stateful_fedgen_aggregator.py:23-33`` and used at
``docs/developer/algorithm/secure_aggregation.ipynb`` cell 16).

Protocol (notebook cell 15, semi-honest, no dropout): every party quantizes
``x*w`` to fixed point ``trunc(x*w*2^fxp)`` (int64 viewed as uint64), adds
``m_uv`` for each peer ``v`` whose name sorts after it and subtracts it
otherwise, where ``m_uv = PCG64(seed_uv).integers(int64.min, int64.max)``;
the server sums the masked uint64 vectors mod 2^64 — the masks cancel — and
decodes ``int64(S) / 2^fxp`` as float64, divided by ``sum(w)`` (or C) for the
average.  All per-element work (quantize, mask expansion, mod-2^64 sums,
decode) runs in the hand-written gfx950 kernels of ``libsfl_sa.so``.

Placement: each party is a ``PYU`` bound to a GPU.  When every party sits on
the server's GPU and the payload is float32 with scalar weights, the clients
are simulated by ONE fused launch (``sa_fused_clients``) that expands each
pair stream once and applies it to both clients; otherwise each party masks
on its own GPU (``sa_mask``), the masked vectors move to the server
(``.to(server)``, the wire) and are summed there (``sa_sum_u64``).  Both give
bit-identical sums.

Small host calls (up to ``SMALL_CALL_BYTES`` a party, co-located parties)
are latency-bound, so each is ONE blocking library call
(``sa_fused_clients_host_f32`` for float32, ``sa_clients_host`` for the
other types: host arrays in, decoded result out); a replay after a flagged
raw 0, wire images, per-element weights or more parties than those calls
take go through the general path above.

Which of these a call takes is decided in one place, ``SecureAggregator._route``
(the route table: DESIGN.md §7); each route is one ``_run_<route>`` method.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from ... import hostpipe as H
from ... import kernels as K
from ... import _lib as L
from ...device import PYU, PYUObject, DeviceObject, reveal
from . import party as P
from .aggregator import Aggregator
from .masker import Masker
from .payload import (F32, F64, I64, SMALL_CALL_BYTES, compute_dtype, element_types, flat_host, host_weight,
                      is_torch, np_dtype, scalar_weight, shape, split_layers, to_device, torch_dtypes)

MAX_FUSED_CLIENTS = 8  # parties of one fused launch (sa_fused_clients, sa_fused_clients_host_f32)
MAX_HOST_CLIENTS = 9   # parties of one sa_clients_host call


class _Rejected(Exception):
    """A masking launch flagged a raw PCG64 draw of 0 (SA_FLAG_PRG_REJECT)."""


@dataclass
class _Call:
    """One aggregation call as the host paths see it: the parties' objects
    and names, their layers (same sizes and shapes for every party), the
    host weights, and how the result goes back (``is_list`` / ``container``:
    the payloads' own kind).  ``C`` parties, ``n`` elements a party.  The
    last six fields are what ``SecureAggregator._route`` decides from."""
    server: PYU
    data: list
    names: list
    layer_lists: tuple
    sizes: list
    shapes: list
    weights: list | None
    average: bool
    is_list: bool
    container: str  # "array" | "list" | "tuple", as party.MaskedPayload names them
    C: int
    n: int
    as_torch: bool       # the payloads are torch tensors (the first layer decides)
    colocated: bool      # every party on the server's GPU
    ldts: set            # the layers' dtypes
    one_dtype_each: bool  # each party's layers are of one dtype
    scalar_w: bool       # every weight absent or a scalar
    cts: set             # the arithmetic types of every (layer dtype, weight)

    def divisor(self) -> float:
        """What the decoded sum is divided by under scalar weights: 1, C or sum(weights)."""
        if not self.average:
            return 1.0
        return float(self.C) if self.weights is None else float(sum(self.weights))

    def scalar_weights(self, ct: np.dtype = F32) -> list:
        """Every party's scalar weight in the kind of the arithmetic type ``ct``."""
        if self.weights is None:
            return [1.0] * self.C
        return [scalar_weight(w, ct) for w in self.weights]

    def pack(self, layers: list) -> PYUObject:
        """The per-layer results in the payloads' container, on the server."""
        if not self.is_list:
            return PYUObject(self.server, layers[0])
        return PYUObject(self.server, tuple(layers) if self.container == "tuple" else layers)

    def wrap(self, flat: np.ndarray) -> PYUObject:
        """A flat host result split into the layers' shapes, packed."""
        parts = np.split(flat, np.cumsum(self.sizes)[:-1]) if len(self.sizes) > 1 else [flat]
        return self.pack([p.reshape(sh) for p, sh in zip(parts, self.shapes)])


@dataclass
class _Group:
    """One launch group: ``n`` elements a party, and per party its device
    vector, arithmetic type, scalar weight and per-element weight vector
    (None under a scalar weight)."""
    n: int
    xs: list
    cts: list
    ws: list
    wvecs: list


class SecureAggregator(Aggregator):
    """Pairwise-mask secure aggregation with the HIP hot path.

    Args:
        device: the server PYU that receives the masked vectors and decodes.
        participants: the client PYUs (distinct parties).
        fxp_bits: fixed-point fraction bits (reference default 18).
        seeds: optional ``{(party_a, party_b): seed}`` pairwise seeds (both
            orders accepted; a ``(state, inc)`` tuple is an explicit numpy
            PCG64 state); default is a Diffie-Hellman agreement.
        fused: allow the single-launch simulation of co-located clients.
        keep_masked: also materialise every party's masked vector (the wire
            image) and expose the last ones as ``last_masked``; co-located
            parties still take the fused launch, which stores the images.

    ``last_digests``: per launch group of the last aggregation, the XOR
    digest of every party's masked vector (a checksum the tests pin) -- None
    for a group of more co-located parties than one launch holds, whose
    pair-shared schedule forms only the masked sum.
    """

    def __init__(self, device: PYU, participants: List[PYU], fxp_bits: int = 18, *,
                 seeds: dict | None = None, fused: bool = True, keep_masked: bool = False):
        assert participants, "participants should not be empty"
        names = [p.party for p in participants]
        assert len(set(names)) == len(names), f"duplicate participants: {names}"
        self._device = device
        self._participants = list(participants)
        self._fxp_bits = int(fxp_bits)
        self._fused = fused
        self._keep_masked = keep_masked
        self.last_masked = None
        self.last_digests = None
        self._careful = False  # replay mode after a flagged rejection (see _aggregate)
        self._scratch = {}  # the one-call library entries' buffers (_call_scratch)
        self._maskers = {n: Masker(n, self._fxp_bits) for n in names}
        if seeds is None:
            keys = {n: m.public_key for n, m in self._maskers.items()}
            for m in self._maskers.values():
                m.agree(keys)
        else:
            for a in names:
                for b in names:
                    if a != b:
                        s = seeds.get((a, b), seeds.get((b, a)))
                        if s is None:
                            raise ValueError(f"missing seed for pair ({a}, {b})")
                        if isinstance(s, tuple):  # an explicit numpy PCG64 (state, inc)
                            self._maskers[a].set_state(b, *s)
                        else:
                            self._maskers[a].set_seed(b, int(s))

    @property
    def device(self) -> PYU:
        return self._device

    @property
    def participants(self) -> List[PYU]:
        return list(self._participants)

    # ------------------------------------------------------------------ API
    def sum(self, data: List[DeviceObject], axis=None) -> DeviceObject:
        return self._aggregate(data, axis, weights=None, average=False)

    def average(self, data: List[DeviceObject], axis=None, weights=None) -> DeviceObject:
        return self._aggregate(data, axis, weights=weights, average=True)

    # ------------------------------------------------------------ internals
    def _aggregate(self, data, axis, weights, average: bool) -> DeviceObject:
        """One aggregation.  The masking kernels only FLAG a raw PCG64 draw
        of 0 (numpy's Generator.integers rejects it and draws again, p =
        2^-64 per draw); when that happens the round is replayed from the
        same stream positions in careful mode, which re-positions the
        affected streams exactly as numpy does (``_fix_rejections``)."""
        snap = {nm: m.snapshot() for nm, m in self._maskers.items()}

        def restore():
            for nm, m in self._maskers.items():
                m.restore(snap[nm])

        try:
            return self._aggregate_once(data, axis, weights, average)
        except _Rejected:
            restore()
        except BaseException:
            # any other failure part-way through a multi-group round: put every
            # stream back where the peers (and numpy) still have it
            restore()
            raise
        self._careful = True
        try:
            return self._aggregate_once(data, axis, weights, average)
        except BaseException:
            restore()
            raise
        finally:
            self._careful = False

    def _aggregate_once(self, data, axis, weights, average: bool) -> DeviceObject:
        call = self._build_call(data, self._validate(data, axis, weights), average)
        return getattr(self, "_run_" + self._route(call))(call)

    def _validate(self, data, axis, weights):
        """The reference's argument checks; returns the weights on the host."""
        assert data, "Data to aggregate should not be None or empty!"
        if axis not in (0, None):
            raise NotImplementedError("SecureAggregator aggregates over parties (axis=0)")
        for d in data:
            assert isinstance(d, PYUObject), f"expect PYUObject, got {type(d)}"
            assert d.device.party in self._maskers, f"{d.device} is not a participant"
        owners = [d.device.party for d in data]
        assert len(set(owners)) == len(owners), "each party may contribute one object"
        assert set(owners) == set(self._maskers), (
            "every participant must contribute (pairwise masks only cancel without dropout, "
            "secure_aggregation.ipynb cell 15)")
        if weights is None:
            return None
        if isinstance(weights, PYUObject):
            raise TypeError("weights must be a per-party list")
        assert len(weights) == len(data), (
            f"Length of the weights does not match the data: {len(weights)} vs {len(data)}.")
        wl = []
        for i, w in enumerate(weights):
            if isinstance(w, PYUObject):
                assert w.device == data[i].device, "Device of weight does not match the corresponding data device."
                w = reveal(w)
            wl.append(host_weight(w))
        return wl

    def _build_call(self, data, weights, average: bool) -> _Call:
        """The ``_Call`` of validated arguments (no GPU work)."""
        layer_lists, containers = zip(*[split_layers(d.data) for d in data])
        nl = len(layer_lists[0])
        for ll in layer_lists:
            assert len(ll) == nl, "parties hold different numbers of arrays"
        shapes = [shape(a) for a in layer_lists[0]]
        for ll in layer_lists:
            assert [shape(a) for a in ll] == shapes, "parties hold arrays of different shapes"
        # layers are masked in order with one stream position per (party, peer),
        # exactly like the reference's per-layer rng.integers calls
        sizes = [int(np.prod(sh)) if sh else 1 for sh in shapes]
        party_dts = [{np_dtype(a) for a in ll} for ll in layer_lists]
        ldts = set().union(*party_dts)
        cts = {compute_dtype(dt, w, self._fxp_bits) for dt in ldts for w in (weights or [None])}
        return _Call(self._device, data, [d.device.party for d in data], layer_lists, sizes, shapes, weights,
                     average, containers[0] != "array", containers[0], len(data), sum(sizes),
                     as_torch=is_torch(layer_lists[0][0]),
                     colocated=all(d.device.gpu == self._device.gpu for d in data), ldts=ldts,
                     one_dtype_each=all(len(s) == 1 for s in party_dts),
                     scalar_w=weights is None or all(np.ndim(w) == 0 for w in weights), cts=cts)

    def _route(self, call: _Call) -> str:
        """The route of one call: the first matching row of the table in
        DESIGN.md §7.  Pure Python on the call's fields and this object's
        switches.  The two sizes that count as large (``4 * n_pad`` for
        float32, ``n * itemsize`` for the general shape) and the two party
        caps (8 and 9) are those of the library entries behind each route."""
        C, n = call.C, call.n
        host = (not call.as_torch and self._fused and not self._keep_masked and n > 0 and C >= 2
                and call.colocated and call.scalar_w)
        # host float32 payloads whose weights keep float32 arithmetic: the
        # fused launch (FL rounds of small models)
        if host and call.ldts == {F32} and call.cts == {F32} and not (C > MAX_FUSED_CLIENTS and self._careful):
            big = 4 * (-(-n // 4) * 4) > SMALL_CALL_BYTES  # rows are padded to 16 bytes
            if big and not self._careful and P.LARGE_PIPELINE:
                return "fused_pipelined"
            if not big and not self._careful and C <= MAX_FUSED_CLIENTS:
                return "fused_one_call"
            return "fused_staged"
        # host payloads of one element type with scalar weights of one
        # arithmetic type (float64 / int64 data, or float32 computed in float64)
        if (host and not self._careful and len(call.ldts) == 1 and len(call.cts) == 1
                and call.ldts <= {F32, F64, I64} and call.cts <= {F32, F64, I64}):
            (xt,) = call.ldts
            if n * xt.itemsize > SMALL_CALL_BYTES:
                if P.LARGE_PIPELINE:
                    return "general_pipelined"
            elif C <= MAX_HOST_CLIENTS:
                return "general_one_call"
        if not call.as_torch and len(call.sizes) > 1 and call.scalar_w and call.one_dtype_each:
            return "general_host_packed"
        return "general"

    # --------------------------------------------- routes: float32, fused launch
    def _staging(self, C: int, n_pad: int, sdev):
        """Pinned host / device buffers reused across rounds of the same size:
        the input block [C, n_pad] float32 (host and device), the masked-sum
        buffer, and one float64 block ``io`` of n_pad + 1 + C words on the
        device with its pinned host mirror -- the decoded result, then a word
        whose low half is the PRG flag word, then the C digests -- so that ONE
        zero fill and ONE device-to-host copy serve all three."""
        key = (C, n_pad, str(sdev))
        st = getattr(self, "_stage", None)
        if st is None or st["key"] != key:
            io_dev = torch.empty(n_pad + 1 + C, dtype=torch.float64, device=sdev)
            io_host = torch.empty(n_pad + 1 + C, dtype=torch.float64, pin_memory=True)
            meta = io_dev[n_pad:].view(torch.int64)
            small = 4 * n_pad <= SMALL_CALL_BYTES  # large calls copy from the caller's arrays
            st = {"key": key,
                  "in_host": torch.empty((C, n_pad) if small else (0, 0), dtype=torch.float32, pin_memory=True),
                  "in_dev": torch.empty((C, n_pad), dtype=torch.float32, device=sdev),
                  "sum": torch.empty(n_pad, dtype=K.U64, device=sdev),
                  "io_dev": io_dev, "io_host": io_host, "meta": meta,
                  "flags": meta[:1].view(torch.int32)[:1], "digests": meta[1:],
                  "io_f64": io_host.numpy(), "io_i64": io_host.numpy().view(np.int64)}
            st["in_np"] = st["in_host"].numpy()
            self._stage = st
        return st

    def _accept(self, call: _Call, flag: int, digests) -> None:
        """The end of a host path's round.  A set PRG flag rejects it before
        any stream has moved (the replay starts from the same positions);
        else every party's streams move on by n and ``digests`` (the one
        launch group's, or None) become ``last_digests``."""
        if flag & L.SA_FLAG_PRG_REJECT:
            raise _Rejected()
        for nm in call.names:
            self._maskers[nm].consume(call.n)
        self.last_digests = [digests]

    def _call_scratch(self, sizes, *args):
        """(pinned, device) scratch of a blocking one-call library entry,
        sized by ``sizes(*args)`` (``kernels.host_fused_scratch`` /
        ``host_clients_scratch``) and kept per entry until its shape changes."""
        sdev = self._device.torch_device
        key = (*args, str(sdev))
        sc = self._scratch.get(sizes)
        if sc is None or sc[0] != key:
            pin_b, dev_b = sizes(*args)
            sc = (key, torch.empty(pin_b, dtype=torch.uint8, pin_memory=True),
                  torch.empty(dev_b, dtype=torch.uint8, device=sdev))
            self._scratch[sizes] = sc
        return sc[1], sc[2]

    def _run_fused_one_call(self, call: _Call):
        """The small call as ONE blocking library call
        (``sa_fused_clients_host_f32``: the parties' layers packed into one
        pinned block, one H2D copy carrying the zeroed PRG flag + digests,
        the fused masking launch -- same kernels and stream positions as the
        general path: bit-identical -- decode, one D2H copy of the result
        with the flag word and the digests, one synchronisation; the Python
        side only positions the pair streams).  The same steps from Python
        (``_run_fused_staged``) when the library has no fused kernel for C."""
        pair_gens, pair_signs = self._pair_streams(call.names)
        pin, dbuf = self._call_scratch(K.host_fused_scratch, call.C, call.n)
        # (a single layer goes as it is: the entry flattens it itself)
        xs = [ll[0] if len(ll) == 1 else flat_host(ll, np.float32) for ll in call.layer_lists]
        with torch.cuda.device(self._device.torch_device):
            got = K.fused_clients_host_f32(xs, call.scalar_weights(), pair_gens, pair_signs, pin, dbuf,
                                           fxp_bits=self._fxp_bits, divisor=call.divisor())
        if got is None:
            return self._run_fused_staged(call)
        out, digests, flag = got
        self._accept(call, flag, torch.from_numpy(digests.view(np.int64)))
        return call.wrap(out)

    def _run_fused_staged(self, call: _Call):
        """The fused launch staged from Python, for what the other two
        float32 routes do not take: a replay (careful mode), a small call of
        more than 8 parties, a large call with ``LARGE_PIPELINE`` off.
        Small calls: one pinned block, one copy each way; large ones copy
        each party's array and the result directly."""
        sdev = self._device.torch_device
        C, n = call.C, call.n
        n_pad = -(-n // 4) * 4  # rows start 16-byte aligned
        # small calls: one pinned block, one copy; large ones: the driver's
        # pageable copy per party (its staging pipelines, a host memcpy into
        # pinned memory first does not)
        big = 4 * n_pad > SMALL_CALL_BYTES
        st = self._staging(C, n_pad, sdev)
        host = st["in_np"]
        with torch.cuda.device(sdev):
            dev_in = st["in_dev"]
            for c, ll in enumerate(call.layer_lists):
                if big:
                    dev_in[c, :n].copy_(H.h2d(flat_host(ll, np.float32), sdev))
                else:
                    flat_host(ll, np.float32, out=host[c, :n])
            if not big:
                dev_in.copy_(st["in_host"], non_blocking=True)
            st["meta"].zero_()
            g = _Group(n, [dev_in[c, :n] for c in range(C)], [F32] * C, call.scalar_weights(), [None] * C)
            s, digests, _ = self._masked_sum(call.data, g, st["flags"], s_out=st["sum"][:n],
                                             digests_out=st["digests"])
            K.decode(s, st["io_dev"][:n], fxp_bits=self._fxp_bits, divisor=call.divisor())
            if big:
                out = H.d2h(st["io_dev"][:n])
                st["io_host"][n_pad:].copy_(st["io_dev"][n_pad:])
            else:
                st["io_host"].copy_(st["io_dev"], non_blocking=True)
                torch.cuda.current_stream(sdev).synchronize()
        io64, ioi = st["io_f64"], st["io_i64"]
        if not big:
            out = io64[:n].copy()
        if int(ioi[n_pad]) & L.SA_FLAG_PRG_REJECT:  # the flag word's low half (little-endian)
            raise _Rejected()
        self.last_digests = [None if digests is None else torch.from_numpy(ioi[n_pad + 1:n_pad + 1 + C].copy())]
        return call.wrap(out)

    def _host_pipelined(self, call: _Call, xt: np.dtype, make_compute, digests: bool):
        """A large host call of co-located parties, chunked through three
        streams (``sfl_amd/hostpipe.py``, as the per-party drop-in's large
        path): chunk j of every party's layers H2D straight from the
        caller's arrays (registered for the call, else staged through pinned
        slots by a feeder thread), the route's masked sum of chunk j on the
        compute stream (``make_compute(x, ssum, meta, bounds)`` returns its
        ``compute(j, lo, hi)``: every stream advanced to ``lo``, the PRG flag
        and the digests accumulated on the device in ``meta``) and its
        decode, then the D2H of chunk j into the result (a recycled
        registered buffer, or a fresh array reached through a pinned slot).
        Bit-identical to one launch over [0, n): the same kernels, the same
        stream positions, element by element.  ``digests``: whether the
        route forms per-party digests."""
        sdev = self._device.torch_device
        C, n, divisor = call.C, call.n, call.divisor()
        layers = [H.host_layers(ll, xt) for ll in call.layer_lists]
        n_pad = -(-n // 4) * 4  # rows 16-byte aligned
        bounds = H.page_bounds(H.chunk_bounds(n), layers)

        def setup():
            x = torch.empty((C, n_pad), dtype=torch_dtypes()[xt], device=sdev)
            ssum = torch.empty(n, dtype=K.U64, device=sdev)
            dec = torch.empty(n, dtype=torch.float64, device=sdev)
            meta = torch.zeros(1 + C, dtype=K.U64, device=sdev)  # flag word | digests
            masked_sum = make_compute(x, ssum, meta, bounds)

            def compute(j, lo, hi):
                masked_sum(j, lo, hi)
                K.decode(ssum[lo:hi], dec[lo:hi], fxp_bits=self._fxp_bits, divisor=divisor)

            copies = [[(x[c, lo:hi], H.pieces(layers[c], lo, hi)) for c in range(C)] for lo, hi in bounds]
            return copies, compute, lambda j: dec[bounds[j][0]:bounds[j][1]], meta

        out, mh = H.run_chunks("average" if call.average else "sum", sdev, bounds, [a for ls in layers for a in ls],
                               np.float64, setup)
        # mh[0]: the flag word's low half (little-endian)
        self._accept(call, int(mh[0]), torch.from_numpy(mh[1:].copy()) if digests else None)
        return call.wrap(out)

    def _run_fused_pipelined(self, call: _Call):
        """Large host float32 payloads: per chunk the fused launch (every
        pair stream advanced to ``lo``); more than 8 parties take the
        pair-shared schedule per chunk (``kernels.fused_many``: the sum only,
        no per-party digests)."""
        C = call.C
        pair_gens, pair_signs = self._pair_streams(call.names)
        ws = call.scalar_weights()
        few = C <= MAX_FUSED_CLIENTS

        def make_compute(x, ssum, meta, bounds):
            flags, digests = meta[:1].view(torch.int32)[:1], (meta[1:] if few else None)

            def compute(j, lo, hi):
                gens = L.pcg64_advance_many(pair_gens, [lo] * len(pair_gens)) if lo else pair_gens
                K.fused_clients([x[c, lo:hi] for c in range(C)], ws, gens, pair_signs, [], 0, ssum[lo:hi],
                                fxp_bits=self._fxp_bits, digests=digests, flags=flags)

            return compute

        return self._host_pipelined(call, F32, make_compute, digests=few)

    def _pair_streams(self, names, want: bool = True):
        """Every internal pair (u < v) of ``names``: its generator at the next
        unused draw (u's view, one library call per party) and u's sign,
        u-major -- the order sa_fused_clients takes."""
        C = len(names)
        gens, signs = [], []
        for u in range(C):
            mu = self._maskers[names[u]]
            later = names[u + 1:]
            for v in later:
                assert mu.position(v) == self._maskers[v].position(names[u]), "pair streams out of step"
            if want and later:
                gens += mu.generators_at(later)
                signs += [mu.sign(v) for v in later]
        return gens, signs

    # ------------------------------- routes: one element type, every party's sa_mask
    def _run_general_one_call(self, call: _Call):
        """Small host calls of float64 / int64 data (or float32 data with a
        float64 compute type) of 2..9 parties on the server's GPU as ONE
        blocking library call (``sa_clients_host``: every party masked with
        its own streams into the sum, decode, one copy each way)."""
        (xt,), (ct,) = call.ldts, call.cts
        streams = [self._maskers[nm].streams(self._maskers[nm].peers) for nm in call.names]
        xs = [flat_host(ll) for ll in call.layer_lists]
        pin, dbuf = self._call_scratch(K.host_clients_scratch, call.C, call.n, xt.itemsize)
        with torch.cuda.device(self._device.torch_device):
            out, digests, flag = K.clients_host(xs, ct, call.scalar_weights(ct), streams, pin, dbuf,
                                                fxp_bits=self._fxp_bits, divisor=call.divisor())
        self._accept(call, flag, torch.from_numpy(digests.view(np.int64)))
        return call.wrap(out)

    def _run_general_pipelined(self, call: _Call):
        """Large host payloads of the same shape, any number of parties:
        per chunk, on the compute stream, every party's ``sa_mask`` with its
        own streams advanced to ``lo`` accumulating into the sum (its digest
        and the PRG flag accumulated on the device)."""
        (xt,), (ct,) = call.ldts, call.cts
        C, tc, ws = call.C, torch_dtypes()[ct], call.scalar_weights(ct)

        def make_compute(x, ssum, meta, bounds):
            masked = torch.empty(max(hi - lo for lo, hi in bounds), dtype=K.U64, device=x.device)
            flags = meta[:1].view(torch.int32)[:1]

            def compute(j, lo, hi):
                streams = [self._maskers[nm].streams(offset=lo) for nm in call.names]
                ssum[lo:hi].zero_()
                for c in range(C):
                    K.mask(x[c, lo:hi], masked[:hi - lo], streams[c], weight=ws[c], compute_dtype=tc,
                           fxp_bits=self._fxp_bits, sum_accum=ssum[lo:hi], digest=meta[1 + c:2 + c], flags=flags)

            return compute

        return self._host_pipelined(call, xt, make_compute, digests=True)

    # ------------------------------------------------- routes: the general path
    def _run_general_host_packed(self, call: _Call):
        """Host layers of one dtype a party under scalar weights: packed on
        the host, one H2D copy per party, ONE launch group."""
        flags = torch.zeros(1, dtype=torch.int32, device=self._device.torch_device)
        flat = [flat_host(ll) for ll in call.layer_lists]
        g = self._prepare_layer(call.data, flat, (call.n,), call.weights)
        return self._finish(call, [(list(range(len(call.sizes))), call.sizes, g)], flags)

    def _run_general(self, call: _Call):
        """Everything else: every layer to its party's GPU, one launch group a layer or one for all."""
        data, layer_lists, sizes = call.data, call.layer_lists, call.sizes
        nl = len(sizes)
        flags = torch.zeros(1, dtype=torch.int32, device=self._device.torch_device)
        prepared = [self._prepare_layer(data, [ll[li] for ll in layer_lists], call.shapes[li], call.weights)
                    for li in range(nl)]
        # Consecutive layers draw consecutive stream positions, so when every
        # layer of a party has the same element/arithmetic type and a scalar
        # weight, the layers are packed into one contiguous vector per party
        # (List[array] <-> one vector + offsets) and aggregated
        # by ONE launch -- bit-identical to the per-layer launches.
        packable = nl > 1 and all(
            all(p.wvecs[ci] is None and p.xs[ci].dtype == prepared[0].xs[ci].dtype
                and p.cts[ci] == prepared[0].cts[ci] for p in prepared)
            for ci in range(len(data)))
        if packable:
            groups = [(list(range(nl)), sizes, _Group(
                sum(sizes), [torch.cat([p.xs[ci] for p in prepared]) for ci in range(len(data))],
                prepared[0].cts, prepared[0].ws, [None] * len(data)))]
        else:
            groups = [([li], [prepared[li].n], prepared[li]) for li in range(nl)]
        return self._finish(call, groups, flags)

    def _finish(self, call: _Call, groups, flags):
        """Masked sum + decode of every launch group, split back into layers."""
        sdev = self._device.torch_device
        data, shapes, weights = call.data, call.shapes, call.weights
        out_layers = [None] * len(shapes)
        host_groups, masked_keep, digests_keep = [], [], []
        for lis, sizes, g in groups:
            n = g.n
            s, digests, masked = self._masked_sum(data, g, flags)
            digests_keep.append(digests)
            if self._keep_masked and len(lis) > 1:  # a packed group's wire images, layer by layer
                bounds = np.cumsum([0] + sizes)
                for k in range(len(lis)):
                    masked_keep.append([m[bounds[k]:bounds[k + 1]] for m in masked])
            elif self._keep_masked:
                masked_keep.append(masked)

            # decode on the server GPU: / 2^fxp, then / C or / sum(w)
            dec = torch.empty(n, dtype=torch.float64, device=sdev)
            divisor, divisor_vec = 1.0, None
            if call.average and not call.scalar_w:
                li = lis[0]
                wb = [H.h2d(np.broadcast_to(np.asarray(w), shapes[li]).astype(np.float64).reshape(-1), sdev)
                      for w in weights]
                divisor_vec = K.sum_f64(wb, torch.empty(n, dtype=torch.float64, device=sdev))
            else:
                divisor = call.divisor()
            K.decode(s, dec, fxp_bits=self._fxp_bits, divisor=divisor, divisor_vec=divisor_vec)
            if call.as_torch:
                for li, part in zip(lis, dec.split(sizes)):
                    out_layers[li] = part.reshape(shapes[li])
            elif 8 * n > SMALL_CALL_BYTES:
                vals = H.d2h(dec)
                for li, part in zip(lis, np.split(vals, np.cumsum(sizes)[:-1])):
                    out_layers[li] = part.reshape(shapes[li])
            else:  # small host results: pinned copies, collected after ONE synchronisation below
                host = torch.empty(n, dtype=torch.float64, pin_memory=True)
                host.copy_(dec, non_blocking=True)
                host_groups.append((lis, sizes, host))

        if not host_groups:
            rejected = int(flags.item()) & L.SA_FLAG_PRG_REJECT
        else:
            fl_host = torch.empty(1, dtype=torch.int32, pin_memory=True)
            fl_host.copy_(flags, non_blocking=True)
            torch.cuda.current_stream(sdev).synchronize()
            rejected = int(fl_host[0]) & L.SA_FLAG_PRG_REJECT
            for lis, sizes, host in host_groups:
                vals = host.numpy().copy()
                for li, part in zip(lis, np.split(vals, np.cumsum(sizes)[:-1]) if len(lis) > 1 else [vals]):
                    out_layers[li] = part.reshape(shapes[li])
        if rejected:
            raise _Rejected()
        if self._keep_masked:
            self.last_masked = masked_keep
        self.last_digests = digests_keep
        return call.pack(out_layers)

    def _prepare_layer(self, data, arrays, shape, weights) -> _Group:
        """Per-party device vector, arithmetic type and weight of one layer."""
        n = int(np.prod(shape)) if shape else 1
        g = _Group(n, [], [], [], [])
        packed = self._pack_host(data, arrays, n)
        for ci, d in enumerate(data):
            party = d.device
            a = arrays[ci]
            w = None if weights is None else weights[ci]
            xt, ct = element_types(np_dtype(a), w, self._fxp_bits)
            x = packed[ci] if packed.get(ci) is not None and packed[ci].dtype == torch_dtypes()[xt] else \
                to_device(a, xt, party.torch_device)
            wv, wscalar = None, 1.0
            if w is not None:
                if np.ndim(w) == 0:
                    wscalar = scalar_weight(w, ct)
                else:
                    wb = np.broadcast_to(np.asarray(w), shape).astype(ct)
                    wv = H.h2d(wb.reshape(-1), party.torch_device)
            g.xs.append(x)
            g.cts.append(ct)
            g.ws.append(wscalar)
            g.wvecs.append(wv)
        return g

    @staticmethod
    def _pack_host(data, arrays, n) -> dict:
        """Host (numpy) arrays of parties on one GPU with one element type:
        packed into one pinned block, ONE host-to-device copy per GPU (the
        small calls of secondary callers, e.g. HomoBinning's counts, are
        bound by per-copy latency).  Returns {party index: device row}."""
        groups = {}
        for ci, d in enumerate(data):
            a = arrays[ci]
            if isinstance(a, torch.Tensor) or n == 0:
                continue
            a = np.asarray(a)
            if a.dtype not in torch_dtypes() or n * a.dtype.itemsize > SMALL_CALL_BYTES:
                continue
            groups.setdefault((d.device.torch_device, a.dtype), []).append(ci)
        rows = {}
        for (dev, dt), cis in groups.items():
            if len(cis) < 2:
                continue
            per = 16 // dt.itemsize
            n_pad = -(-n // per) * per  # every row 16-byte aligned
            host = torch.empty((len(cis), n_pad), dtype=torch_dtypes()[dt], pin_memory=True)
            hv = host.numpy()
            for r, ci in enumerate(cis):
                hv[r, :n] = np.asarray(arrays[ci]).reshape(-1)
            dv = host.to(dev, non_blocking=True)
            for r, ci in enumerate(cis):
                rows[ci] = dv[r, :n]
        return rows

    def _masked_sum(self, data, g: _Group, flags, *, s_out=None, digests_out=None):
        """One launch group's masked sum on the server GPU.  Returns (sum,
        per-party digests or None, materialised masked vectors or None).
        ``s_out`` / ``digests_out``: preallocated sum (n) and zeroed digest
        (C) buffers on the server GPU (the host latency path's staging)."""
        server = self._device
        sdev = server.torch_device
        parties = [d.device for d in data]
        names = [p.party for p in parties]
        C, n = len(names), g.n
        s = torch.empty(n, dtype=K.U64, device=sdev) if s_out is None else s_out
        # more co-located parties than one launch holds: the pair-shared
        # multi-launch schedule (kernels.fused_many), which forms only the sum
        # (no per-party digests; wire images and the careful replay take the
        # per-party path below)
        many = C > MAX_FUSED_CLIENTS
        if many:
            digests = None
        else:
            digests = torch.zeros(C, dtype=K.U64, device=sdev) if digests_out is None else digests_out
        fusable = (self._fused and C >= 2 and (not many or not (self._keep_masked or self._careful))
                   and all(p.gpu == server.gpu for p in parties)
                   and all(ct == F32 for ct in g.cts)
                   and all(x.dtype == torch.float32 for x in g.xs)
                   and all(wv is None for wv in g.wvecs)
                   and set(names) == set(self._maskers))
        # the pair streams (one host jump-ahead each) only where a path uses
        # them: the fused launch and the careful replay's rejection search
        want_pairs = fusable or self._careful
        pair_gens, pair_signs = self._pair_streams(names, want_pairs)
        # per-party (generator, sign, peer) lists: the wire path's launches and the
        # careful-mode rejection fix-up need them (built lazily: 7 jump-aheads a party)
        client_streams = (None if fusable and not self._careful else
                          [self._maskers[p.party].streams(self._maskers[p.party].peers) for p in parties])
        if fusable:
            # keep_masked: the same launch also stores every party's masked
            # vector (the wire image) -- pair streams are still expanded once
            masked = [torch.empty(n, dtype=K.U64, device=sdev) for _ in range(C)] if self._keep_masked else None
            with torch.cuda.device(sdev):
                K.fused_clients(g.xs, g.ws, pair_gens, pair_signs, [], 0, s, fxp_bits=self._fxp_bits,
                                digests=digests, flags=flags, masked_outs=masked)
        else:
            if digests is None:
                digests = torch.zeros(C, dtype=K.U64, device=sdev) if digests_out is None else digests_out
            masked = []
            for ci, p in enumerate(parties):
                pdev = p.torch_device
                local = pdev == sdev
                out = torch.empty(n, dtype=K.U64, device=pdev)
                # a party on the server's GPU writes its digest and flag in place
                dig = digests[ci:ci + 1] if local else torch.zeros(1, dtype=K.U64, device=pdev)
                fl = flags if local else torch.zeros(1, dtype=torch.int32, device=pdev)
                with torch.cuda.device(pdev):
                    K.mask(g.xs[ci], out, client_streams[ci], weight=g.ws[ci], weight_vec=g.wvecs[ci],
                           compute_dtype=torch_dtypes()[g.cts[ci]], fxp_bits=self._fxp_bits, digest=dig, flags=fl)
                if not local:
                    flags |= fl.to(sdev)
                    digests[ci] = dig.to(sdev)[0]
                masked.append(out if local else out.to(sdev))   # the wire: masked vector to the server
            with torch.cuda.device(sdev):
                K.sum_u64(masked, s)
        # masked: the materialised masked vectors (None: fused launch without wire images)
        extra = {}
        if self._careful:
            torch.cuda.synchronize(sdev)
            if int(flags.item()) & L.SA_FLAG_PRG_REJECT:
                extra = self._fix_rejections(names, pair_gens, pair_signs, client_streams, g, masked, digests, s)
                flags.zero_()
        for ci, p in enumerate(parties):
            self._maskers[p.party].consume(n)
        for (a, b), k in extra.items():  # the rejected raw draws consumed on top
            self._maskers[a].skip(b, k)
            self._maskers[b].skip(a, k)
        return s, digests, masked

    def _fix_rejections(self, names, pair_gens, pair_signs, client_streams, g: _Group, wire, digests, s) -> dict:
        """numpy's rejection re-draw for one launch group (careful mode).

        For every pair stream: the elements from which it runs one more raw
        draw along (``kernels.rejected_draws``); the two clients' masked
        vectors are shifted there (``sa_stream_shift``, opposite signs, so
        the masked sum is unchanged) and their digests recomputed.  Without
        materialised vectors (fused launch, no wire images) an affected
        client's vector is re-masked into scratch for its digest.  Returns
        {(party_a, party_b): extra raw draws} for the stream positions."""
        sdev = self._device.torch_device
        C, n = len(names), g.n
        fixes = {c: [] for c in range(C)}  # client -> [(gen, sign, points)]
        extra = {}
        # one batched search over every pair stream first (64 generators per
        # launch); only streams with a hit are followed further
        found = K.rejected_draws_many(pair_gens, n, sdev)
        p = 0
        for u in range(C):
            for v in range(u + 1, C):
                pts, total = found[p]
                if pts:
                    fixes[u].append((pair_gens[p], pair_signs[p], pts))
                    fixes[v].append((pair_gens[p], -pair_signs[p], pts))
                    extra[(names[u], names[v])] = total - n
                p += 1
        for c in range(C):
            if not fixes[c]:
                continue
            if wire is not None:
                vec = wire[c]
            else:
                vec = torch.empty(n, dtype=K.U64, device=sdev)
                K.mask(g.xs[c], vec, client_streams[c], weight=g.ws[c], weight_vec=g.wvecs[c],
                       compute_dtype=torch_dtypes()[g.cts[c]], fxp_bits=self._fxp_bits)
            for gen, sign, pts in fixes[c]:
                K.stream_shifts(vec, gen, sign, pts)
            digests[c] = 0
            K.xor_digest(vec, digests[c:c + 1])
        if wire is not None:  # the server sums the wire images it received
            K.sum_u64(wire, s)
        return extra
