#!/usr/bin/env python3
"""FreqFed's feature and Gram pass on one GPU: the sa_freq kernels
(sfl_amd/csrc/sa_freq.hip) against the same two float64 products in torch on
the same device, and against the reference's per-row ``dct`` and filter loop
on the host, for --clients float32 clients and one layer shape a line: a
``(10, 512)`` head and a ``(1000, 2048)`` fc layer (synthetic seeded weights).

* hip:   ``freq_features`` (basis, two products) and ``freq_gram`` into device
         buffers (no read-back in the figure)
* torch: ``A @ (W.double() @ B.T)`` batched over the clients with the basis
         precomputed outside the figure, the filter as a multiply by a 0/1
         mask, ``F @ F.T`` for the Gram matrix
* host:  agg_freqfed.py's ``tensorDCT`` and ``filtering`` (scipy ``dct`` per row
         and per column, the Python double loop) for one client on one core,
         scaled by --clients; timed once with a host clock (it takes seconds).
         Skipped where scipy is missing.

hip and torch alternate inside every pass (--reps calls each, after a warm-up
of both on these shapes); a figure is the median over the passes of the
per-pass median, timed with device events.  One JSON line a shape:

  hip_ms, torch_ms, host_ms; speedup_vs_torch, speedup_vs_host (other / hip:
    below 1 is not a gain);
  flops_model: 2 M N wk + 2 hk M wk a client; that over hip_ms as TFLOP/s and
    as a fraction of FP64_MATRIX_PEAK_TFLOPS;
  bytes_model: W read once, the first product written and read, the features
    written and read by the Gram pass, the basis written and read; that over
    hip_ms as GB/s and as a fraction of benchkit/roofline's HBM peak;
  max_ratio_vs_torch: the largest |hip - torch| of a feature over the tests'
    tolerance (M + N + 16) 2^-53 ||W||_F.

usage: python tools/freq_bench.py [--clients 8] [--reps 10] [--passes 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MATRIX_PEAK_TFLOPS = 78.6  # the MI355X data sheet's float64 matrix rate
SHAPES = {"head": (10, 512), "fc": (1000, 2048)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freq", "freq_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import _lib as L
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.security.aggregation import freq_aggregator as F

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("freq_bench: needs a GPU (no fallback)")
    dev = torch.device("cuda", 0)
    C = args.clients
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

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

    for name, (M, N) in SHAPES.items():
        hk, wk, q = F.corner(M, N)
        g = torch.Generator(device=dev).manual_seed(23)
        ws = [(torch.randn((M, N), generator=g, device=dev) * 0.05).reshape(-1) for _ in range(C)]
        scratch = torch.empty(K.freq_scratch_bytes(M, N, C, torch.float32), dtype=torch.uint8, device=dev)
        feats = torch.empty(C * hk * wk, dtype=torch.float64, device=dev)
        gram = torch.empty(C * (C + 1) // 2, dtype=torch.float64, device=dev)
        A, B = H.h2d(F.basis_host(hk, M), dev), H.h2d(F.basis_host(wk, N), dev)
        i, j = np.arange(hk)[:, None], np.arange(wk)[None, :]
        mask = H.h2d((i + j <= q).astype(np.float64), dev)
        W3 = torch.stack([w.reshape(M, N) for w in ws])
        keep = {}

        def hip():
            K.freq_features(ws, M, N, scratch, feats)
            K.freq_gram(feats, C, hk * wk, gram)

        def torch_pass():
            f = (A @ (W3.double() @ B.T)) * mask
            keep["f"] = f
            keep["g"] = f.reshape(C, -1) @ f.reshape(C, -1).T

        hip(), torch_pass()  # warm-up of both on these shapes
        torch.cuda.synchronize()
        hs, ts = [], []
        for _ in range(args.passes):
            hs.append(events(hip, args.reps))
            ts.append(events(torch_pass, args.reps))
        hip_ms, torch_ms = statistics.median(hs), statistics.median(ts)
        got = H.d2h(feats, pooled=False).reshape(C, hk, wk)
        ref = H.d2h(keep["f"].contiguous(), pooled=False)
        norms = [float(np.linalg.norm(H.d2h(w, pooled=False).astype(np.float64))) for w in ws]
        ratio = max(float(np.abs(got[c] - ref[c]).max()) / ((M + N + 16) * 2.0 ** -53 * norms[c]) for c in range(C))

        host_ms = None
        if not args.skip_host:
            try:
                from scipy.fftpack import dct
            except ImportError:
                dct = None
            if dct is not None:
                w0 = H.d2h(ws[0], pooled=False).reshape(M, N)
                t0 = time.perf_counter()
                rows = np.array([dct(r, type=2, norm="ortho") for r in w0])
                V = np.array([dct(c, type=2, norm="ortho") for c in rows.T]).T
                sub = V[:M // 2, :N // 2]
                _ = [sub[a][b] for a in range(M // 2) for b in range(N // 2) if a + b <= q]
                host_ms = (time.perf_counter() - t0) * 1e3 * C

        flops = C * (2 * M * N * wk + 2 * hk * M * wk)
        model = C * (M * N * 4 + 2 * wk * M * 8 + 2 * hk * wk * 8) + 2 * (hk * M + wk * N) * 8
        tflops, gbps = flops / (hip_ms * 1e-3) / 1e12, model / (hip_ms * 1e-3) / 1e9
        line = {"case": "features+gram", "layer": name, "shape": [M, N], "corner": [hk, wk, q], "dtype": "float32",
                "clients": C, "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4),
                "host_ms": None if host_ms is None else round(host_ms, 1),
                "speedup_vs_torch": round(torch_ms / hip_ms, 2),
                "speedup_vs_host": None if host_ms is None else round(host_ms / hip_ms, 1),
                "hip_ms_passes": [round(x, 4) for x in hs], "torch_ms_passes": [round(x, 4) for x in ts],
                "launches": 4, "flops_model": flops, "model_tflops": round(tflops, 3),
                "model_frac_fp64_matrix_peak": round(tflops / FP64_MATRIX_PEAK_TFLOPS, 4), "bytes_model": model,
                "model_gbps": round(gbps, 1), "model_frac_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4),
                "max_ratio_vs_torch": ratio, "timer": "device events; host: perf_counter",
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
