#!/usr/bin/env python3
"""The COO transport on one GPU: the sa_coo kernels (sfl_amd/csrc/sa_coo.hip)
against the torch composition a user would write on the same device, and
against the host (numpy) path at a size it finishes quickly, on the same
seeded data in one process.

Cases at --elems float32 elements, densities 0.01 and 0.1:
* encode: count + one pinned read of nnz + allocation + fill (sparse_encode's
          device path) against nonzero + gather; encode_kernels is count and
          fill alone (nnz known, outputs allocated), timed with device events
* decode: memset + validated scatter against zeros + index_put_
* sum:    the sparse average of --parties such uploads (zero the accumulator,
          one axpy per party, one division) against the dense average (K
          dense adds, one division) and against decoding every upload and
          adding it

The implementations alternate inside every pass (--reps / --torch-reps calls
each, after a warm-up of both on the case's shapes); a case's figure is the
median over the passes of the per-pass median.  encode is timed with the host
clock around a call that ends in the blocking read (device events cannot see
the host's part); everything else with device events.  One JSON line per case:

  hip_ms, torch_ms, speedup (torch_ms / hip_ms), host_ms at host_elems;
  bytes_model: encode reads 2 n s and writes nnz (4 + s); decode writes n s
    and reads nnz (4 + s); the sum touches n sA (zeroing), 2 n sA (division)
    and, per party, nnz_k (4 + s) read plus 2 nnz_k sA of accumulator traffic
    -- reported as the issue's lower bound n sA + sum nnz_k (4 + s) and as
    what the passes move;
  both over hip_ms as GB/s and as a fraction of benchkit/roofline's HBM peak;
  same: the two implementations gave the same bits.

usage: python tools/coo_bench.py [--elems 100000000] [--parties 8] [--host-elems 4000000]
                                 [--reps 10] [--torch-reps 3] [--passes 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", type=int, default=100_000_000)
    ap.add_argument("--parties", type=int, default=8)
    ap.add_argument("--host-elems", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coo", "coo_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import _lib as L
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.utils import sparse as S

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("coo_bench: needs a GPU (no fallback)")
    dev = torch.device("cuda", 0)
    n, kp, s = args.elems, args.parties, 4

    def events(fn, reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    def clock(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def host_clock(fn, reps=3):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def ab(hip, other, timer):
        hip(), other()  # warm-up of both on these shapes
        torch.cuda.synchronize()
        hs, ts = [], []
        for _ in range(args.passes):
            hs.append(timer(hip, args.reps))
            ts.append(timer(other, args.torch_reps))
        return statistics.median(hs), statistics.median(ts), hs, ts

    def make(m, density, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        x = torch.randn(m, generator=g, device=dev, dtype=torch.float32)
        return x * (torch.rand(m, generator=g, device=dev) < density)

    lines = []

    def emit(case, density, hip_ms, torch_ms, hs, ts, model, moved, same, host, **extra):
        gbps = lambda b: b / (hip_ms * 1e-3) / 1e9  # noqa: E731
        line = {"case": case, "elems": n, "density": density, "hip_ms": round(hip_ms, 4),
                "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / hip_ms, 2),
                "hip_ms_passes": [round(x, 4) for x in hs], "torch_ms_passes": [round(x, 4) for x in ts],
                "bytes_model": model, "model_gbps": round(gbps(model), 1),
                "model_frac_hbm_peak": round(gbps(model) / HBM_PEAK_GBPS, 4),
                "bytes_moved": moved, "moved_gbps": round(gbps(moved), 1),
                "moved_frac_hbm_peak": round(gbps(moved) / HBM_PEAK_GBPS, 4), "same": same,
                "host_elems": args.host_elems, "host_ms": None if host is None else round(host, 3),
                "device": torch.cuda.get_device_name(0)}
        line.update(extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for density in (0.01, 0.1):
        x = make(n, density, 7)
        hx = H.d2h(make(args.host_elems, density, 7), pooled=False)
        keep = {}

        # ---------------------------------------------------------------- encode
        def hip_encode():
            keep["c"] = S.sparse_encode([x])[0]

        def torch_encode():
            idx = torch.nonzero(x).reshape(-1)
            keep["t"] = (idx.to(torch.int32), x[idx])

        hip_ms, torch_ms, hs, ts = ab(hip_encode, torch_encode, clock)
        c = keep["c"]
        nnz = c.nnz
        same = bool(torch.equal(c.index, keep["t"][0]) and torch.equal(c.data.view(torch.int32),
                                                                       keep["t"][1].view(torch.int32)))
        host_enc = host_clock(lambda: S.sparse_encode([hx]))
        model = 2 * n * s + nnz * (4 + s)
        emit("encode", density, hip_ms, torch_ms, hs, ts, model, model, same, host_enc, nnz=nnz, timer="host clock",
             launches=3)

        scratch = torch.empty(K.coo_scratch_bytes(n, x.dtype) // 4, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        index, data, flag = torch.empty_like(c.index), torch.empty_like(c.data), K.coo_flag(dev)

        def hip_kernels():
            K.coo_count(x, scratch, count)
            K.coo_fill(x, scratch, index, data, flag)

        hip_ms, torch_ms, hs, ts = ab(hip_kernels, torch_encode, events)
        same = bool(torch.equal(index, c.index) and torch.equal(data.view(torch.int32), c.data.view(torch.int32))
                    and H.d2h(flag, pooled=False).tolist() == [0, -1])
        emit("encode_kernels", density, hip_ms, torch_ms, hs, ts, model, model, same, None, nnz=nnz,
             timer="device events", launches=3)

        # ---------------------------------------------------------------- decode
        dense = torch.empty(n, dtype=x.dtype, device=dev)
        long_index = c.index.to(torch.int64)  # index_put_ wants int64: converted outside the timed call

        def hip_decode():
            K.coo_decode(c.index, c.data, dense, flag)

        def torch_decode():
            keep["d"] = torch.zeros(n, dtype=x.dtype, device=dev).index_put_((long_index,), c.data)

        hip_ms, torch_ms, hs, ts = ab(hip_decode, torch_decode, events)
        same = bool(torch.equal(dense.view(torch.int32), keep["d"].view(torch.int32))
                    and H.d2h(flag, pooled=False).tolist() == [0, -1])
        hc = S.sparse_encode([hx])[0]
        host_dec = host_clock(lambda: S.sparse_decode([hc]))
        model = n * s + nnz * (4 + s)
        emit("decode", density, hip_ms, torch_ms, hs, ts, model, model, same, host_dec, nnz=nnz,
             timer="device events", launches=2)
        keep.clear()
        del dense, long_index, index, data

        # ------------------------------------------------------------------- sum
        ups = [S.sparse_encode([make(n, density, 100 + k)])[0] for k in range(kp)]
        nnzs = [u.nnz for u in ups]
        w = [float(32 + 7 * k) for k in range(kp)]  # FLModel's sample counts: A = float64
        acc = torch.empty(n, dtype=torch.float64, device=dev)
        flags = torch.zeros((kp, 2), dtype=torch.int32, device=dev)
        flags[:, 1] = -1

        def hip_sum():
            acc.zero_()
            for k, u in enumerate(ups):
                K.coo_axpy(u.index, u.data, w[k], acc, flags[k])
            K.coo_finish(acc, sum(w))

        # a tensor divisor: torch divides by a python scalar as a multiplication by its reciprocal
        total = torch.zeros((), dtype=torch.float64, device=dev) + sum(w)
        dense_ups = None
        if n * s * kp <= 8 << 30:  # the dense uploads side by side: what a dense transport would hold
            dense_ups = [S.sparse_decode([u])[0] for u in ups]

        def torch_dense_sum():
            t = torch.zeros(n, dtype=torch.float64, device=dev)
            for k, d in enumerate(dense_ups):
                t.add_(d.to(torch.float64) * w[k])
            keep["s"] = t.div_(total)

        def torch_decode_sum():
            t = torch.zeros(n, dtype=torch.float64, device=dev)
            for k, u in enumerate(ups):
                d = torch.zeros(n, dtype=x.dtype, device=dev).index_put_((u.index.to(torch.int64),), u.data)
                t.add_(d.to(torch.float64) * w[k])
            keep["s"] = t.div_(total)

        other = torch_dense_sum if dense_ups is not None else torch_decode_sum
        hip_ms, torch_ms, hs, ts = ab(hip_sum, other, events)
        same = bool(torch.equal(acc.view(torch.int64), keep["s"].view(torch.int64))
                    and not H.d2h(flags, pooled=False)[:, 0].any())
        keep.clear()
        decode_ms = events(torch_decode_sum, args.torch_reps) if dense_ups is not None else torch_ms
        keep.clear()
        from sfl_amd.device import PYU, PYUObject
        from sfl_amd.security import SparsePlainAggregator

        agg = SparsePlainAggregator(PYU("server", None))
        hobjs = [PYUObject(PYU(f"p{k}", None), [S.sparse_encode([H.d2h(make(args.host_elems, density, 100 + k),
                                                                      pooled=False)])[0]]) for k in range(kp)]
        host_sum = host_clock(lambda: agg.average(hobjs, axis=0, weights=[int(v) for v in w]))
        sa = 8
        model = n * sa + sum(nnzs) * (4 + s)
        moved = 3 * n * sa + sum(nnzs) * (4 + s + 2 * sa)
        emit("sum", density, hip_ms, torch_ms, hs, ts, model, moved, same, host_sum, parties=kp, nnz=nnzs,
             torch_is="dense adds" if dense_ups is not None else "decode and add",
             torch_decode_and_add_ms=round(decode_ms, 4), timer="device events", launches=kp + 2)
        del ups, dense_ups, acc, x
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
