#!/usr/bin/env python3
"""FLAME aggregation on one GPU: the sa_flame kernels
(sfl_amd/csrc/sa_flame.hip) against the same arithmetic in torch ops on the
same device, on the same seeded data in one process.

Cases at --elems elements per client: float32 at C = 8 and C = 16 clients,
float64 at C = 8.
* stats:    sa_flame_stats (median, update norms, Gram matrix; one pass up to
            8 clients, two above) against stack / sort(dim=0) / middle rows,
            sub, square().sum(dtype=float64) and X @ X.T in float64
* combine:  sa_flame_combine against the scaled weighted sum in torch ops
* together: both, back to back, with fixed decisions between them (the host's
            read of the statistics is not in the figure)

The torch chain needs the stacked clients in float64 for its Gram matrix; at
--elems it is run in --torch-chunks column chunks so that it fits beside the
data, and its figure is the sum over the chunks.  The implementations
alternate inside every pass (--reps / --torch-reps calls each, after a warm-up
of both); a case's figure is the median over the passes of the per-pass median,
timed with device events.  One JSON line per case:

  hip_ms, torch_ms, speedup (torch_ms / hip_ms): below 1 is not a gain;
  bytes_model: stats C n s read + n s written per pass over the clients (the
    second pass reads the clients of its rows only and writes nothing);
    combine (C_kept + 1) n s + 8 n;
  that over hip_ms as GB/s and as a fraction of benchkit/roofline's HBM peak;
  fma_model (stats): n C (C + 1) / 2 + n C float64 FMAs, and those per second;
  same: the median has torch's bits, the statistics agree to 1e-9 relatively,
    the combine to 1e-12.

usage: python tools/flame_bench.py [--elems 100000000] [--reps 5] [--torch-reps 2] [--passes 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--torch-chunks", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flame", "flame_bench.jsonl"))
    args = ap.parse_args()
    import torch

    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("flame_bench: needs a GPU (no fallback)")
    dev = torch.device("cuda", 0)
    n = args.elems

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

    def ab(hip, other):
        hip(), other()  # warm-up of both on these shapes
        torch.cuda.synchronize()
        hs, ts = [], []
        for _ in range(args.passes):
            hs.append(events(hip, args.reps))
            ts.append(events(other, args.torch_reps))
        return statistics.median(hs), statistics.median(ts), hs, ts

    lines = []

    def emit(case, dtype, C, hip_ms, torch_ms, hs, ts, model, same, **extra):
        gbps = model / (hip_ms * 1e-3) / 1e9
        line = {"case": case, "elems": n, "dtype": dtype, "clients": C, "hip_ms": round(hip_ms, 4),
                "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / hip_ms, 2),
                "hip_ms_passes": [round(x, 4) for x in hs], "torch_ms_passes": [round(x, 4) for x in ts],
                "bytes_model": model, "model_gbps": round(gbps, 1),
                "model_frac_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4), "same": same, "timer": "device events",
                "device": torch.cuda.get_device_name(0)}
        line.update(extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for tdt, C in ((torch.float32, 8), (torch.float32, 16), (torch.float64, 8)):
        g = torch.Generator(device=dev).manual_seed(11)
        xs = [torch.randn(n, generator=g, device=dev, dtype=tdt) for _ in range(C)]
        s = xs[0].element_size()
        name = str(tdt).replace("torch.", "")
        S = K.flame_stat_count(C)
        median = torch.empty(n, dtype=tdt, device=dev)
        scratch = torch.empty(K.flame_scratch_bytes(n, C, tdt), dtype=torch.uint8, device=dev)
        stats = torch.zeros(S, dtype=torch.float64, device=dev)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        # fixed decisions: every second client clipped, the last one left out
        scales = [1.0 if i % 2 else 0.37 for i in range(C)]
        weights = [float(3 + i) for i in range(C)]
        keep = [i != C - 1 for i in range(C)]
        W = sum(w for w, k in zip(weights, keep) if k)
        kept = sum(keep)
        bounds = [(n * i // args.torch_chunks, n * (i + 1) // args.torch_chunks) for i in range(args.torch_chunks)]
        keepers = {}

        def hip_stats():
            K.flame_stats(xs, median, scratch, stats)

        def torch_stats():
            gram = torch.zeros((C, C), dtype=torch.float64, device=dev)
            norms = torch.zeros(C, dtype=torch.float64, device=dev)
            meds = []
            for lo, hi in bounds:
                X = torch.stack([x[lo:hi] for x in xs])
                srt = torch.sort(X, dim=0).values
                med = srt[C // 2] if C % 2 else (srt[C // 2 - 1] + srt[C // 2]) / 2
                norms += (X - med).square().sum(dim=1, dtype=torch.float64)
                X64 = X.to(torch.float64)
                gram += X64 @ X64.T
                meds.append(med)
            keepers["t"] = (meds, gram, norms)

        def hip_combine():
            K.flame_combine(xs, scales, weights, keep, median, W, out)

        def torch_combine():
            outs = []
            for lo, hi in bounds:
                med = median[lo:hi]
                acc = torch.zeros(hi - lo, dtype=torch.float64, device=dev)
                for x, sc, w, k in zip(xs, scales, weights, keep):
                    if k:
                        acc += (med + (x[lo:hi] - med) * sc).to(torch.float64) * w
                outs.append(acc / W + 0.0)
            keepers["c"] = outs

        def hip_both():
            hip_stats(), hip_combine()

        def torch_both():
            torch_stats(), torch_combine()

        passes = 1 if C <= 8 else 2
        second = 0
        if passes == 2:  # the second pass reads the clients of its rows only (sa_flame.hip first_rows)
            r, have = 0, 0
            while 2 * have < C * (C + 1) // 2:
                have, r = have + C - r, r + 1
            second = (C - r) * n * s
        stats_model = C * n * s + n * s + second
        combine_model = (kept + 1) * n * s + 8 * n
        fmas = n * (C * (C + 1) // 2 + C)

        hip_ms, torch_ms, hs, ts = ab(hip_stats, torch_stats)
        meds, gram, norms = keepers["t"]
        iu = torch.triu_indices(C, C, device=dev)
        want = torch.cat([gram[iu[0], iu[1]], norms])
        same_median = bool(torch.equal(torch.cat(meds).view(torch.uint8), median.view(torch.uint8)))
        same = same_median and bool(torch.allclose(stats, want, rtol=1e-9, atol=0))
        emit("stats", name, C, hip_ms, torch_ms, hs, ts, stats_model, same, launches=passes + 1, passes_over_x=passes,
             fma_model=fmas, gfma_per_s=round(fmas / (hip_ms * 1e-3) / 1e9, 1), same_median=same_median)

        hip_ms, torch_ms, hs, ts = ab(hip_combine, torch_combine)
        same = bool(torch.allclose(out, torch.cat(keepers["c"]), rtol=1e-12, atol=0))
        emit("combine", name, C, hip_ms, torch_ms, hs, ts, combine_model, same, launches=1, kept=kept)

        hip_ms, torch_ms, hs, ts = ab(hip_both, torch_both)
        emit("together", name, C, hip_ms, torch_ms, hs, ts, stats_model + combine_model, same, launches=passes + 2,
             kept=kept)
        keepers.clear()
        del xs, median, out
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
