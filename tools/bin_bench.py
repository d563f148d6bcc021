#!/usr/bin/env python3
"""HomoBinning's local passes on one GPU: the sa_bin kernels (sfl_amd/csrc/
sa_bin.hip) against the two other ways to the same counts on the same device,
on the same seeded data in one process.

Cases: float32, --rows x 64 features, Q = 10, 64 and 255 query points a feature.
* ranks:  one ``sa_bin_ranks`` pass (device events) against
          (a) ``hist``: what the library offered before: ``FeatureHistogram.
              bind`` + ``set_gradients(zeros)`` + ``calculate_histogram`` of one
              node, whose N column is the rank; the codes pass is included
              because the query points change every round
          (b) ``torch``: ``bucketize`` a feature + ``bincount`` + ``cumsum``
          ``same_counts``: the three tables are equal
* range:  one ``sa_bin_range`` pass against torch's ``amin`` / ``amax`` /
          ``isnan().sum()`` over the rows
* fit:    a whole two-party ``fit_split_points`` on device parties (a tenth and
          nine tenths of the rows), host clock around the blocking call

The implementations alternate inside every pass (--reps / --other-reps calls
each, after a warm-up of all); a figure is the median over the passes of the
per-pass median, and the per-pass medians are kept.  ``bytes_model``: x read
once; its GB/s over benchkit/roofline's HBM peak is ``model_frac_hbm_peak``.

usage: python tools/bin_bench.py [--rows 10000000] [--reps 5] [--other-reps 2] [--passes 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = 64
QS = (10, 64, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--other-reps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin", "bin_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from sfl_amd import _lib as L

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("bin_bench: needs a GPU (no fallback)")
    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.ml.boost import FeatureHistogram
    from sfl_amd.preprocessing.binning import HomoBinning

    dev = torch.device("cuda", 0)
    rows = args.rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def emit(line):
        line.update(dtype="float32", rows=rows, features=F, timer=line.get("timer", "device events"),
                    lib=os.path.basename(L.LIB_PATH), device=torch.cuda.get_device_name(0))
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)

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

    def alternate(ours, *others):
        for fn in (ours,) + others:
            fn()
        torch.cuda.synchronize()
        res = [[] for _ in range(1 + len(others))]
        for _ in range(args.passes):
            res[0].append(events(ours, args.reps))
            for r, fn in zip(res[1:], others):
                r.append(events(fn, args.other_reps))
        return res

    def figures(name, passes):
        return {f"{name}_ms": round(statistics.median(passes), 4), f"{name}_ms_passes": [round(v, 4) for v in passes]}

    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn((rows, F), generator=g, device=dev, dtype=torch.float32)
    model = rows * F * 4
    zeros = torch.zeros(rows, device=dev, dtype=torch.float32)
    node = torch.zeros(rows, device=dev, dtype=torch.int32)
    keep = {}

    for q in QS:
        rng = np.random.default_rng(q)
        table = np.sort(rng.standard_normal((F, q)).astype(np.float32).astype(np.float64), axis=1)
        qd = H.h2d(table, dev)
        q32 = H.h2d(table.astype(np.float32), dev)
        out = torch.empty((F, q), dtype=torch.int64, device=dev)
        fh = FeatureHistogram(list(table))

        def hip_ranks():
            keep["hip"] = K.bin_ranks(x, qd, (), out)

        def hist_ranks():
            codes = fh.bind(x)
            fh.set_gradients(zeros, zeros)
            keep["hist"] = fh.calculate_histogram(codes, node, 1)[0, :, :, 2]

        def torch_ranks():
            keep["torch"] = torch.stack([torch.cumsum(torch.bincount(
                torch.bucketize(x[:, f], q32[f], right=True), minlength=q + 1), 0)[:q] for f in range(F)])

        hip, hist, tch = alternate(hip_ranks, hist_ranks, torch_ranks)
        same = bool((keep["hip"] == keep["hist"].to(torch.int64)).all() and (keep["hip"] == keep["torch"]).all())
        keep.clear()
        torch.cuda.empty_cache()
        form, qp, fg, lds, groups = K.bin_geometry(q, F, torch.float32)
        line = {"case": "ranks", "q": q, "form": "lds" if form else "registers", "padded_q": qp, "feature_group": fg,
                "lds_bytes": lds, "groups": groups}
        line.update(figures("hip", hip), **figures("hist", hist), **figures("torch", tch))
        line.update(speedup_vs_hist=round(line["hist_ms"] / line["hip_ms"], 2),
                    speedup_vs_torch=round(line["torch_ms"] / line["hip_ms"], 2), same_counts=same, bytes_model=model,
                    model_gbps=round(model / (line["hip_ms"] * 1e-3) / 1e9, 1),
                    model_frac_hbm_peak=round(model / (line["hip_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4))
        emit(line)

    r4 = torch.empty((F, 4), dtype=torch.int64, device=dev)

    def hip_range():
        keep["hip"] = K.bin_range(x, (), r4)

    def torch_range():
        keep["torch"] = (x.amin(0), x.amax(0), torch.isnan(x).sum(0))

    hip, tch = alternate(hip_range, torch_range)
    w = H.d2h(keep["hip"], pooled=False)
    same = bool(np.array_equal(w[:, 0].copy().view(np.float64), H.d2h(keep["torch"][0], pooled=False).astype(np.float64))
                and np.array_equal(w[:, 1].copy().view(np.float64),
                                   H.d2h(keep["torch"][1], pooled=False).astype(np.float64)) and (w[:, 2] == rows).all())
    keep.clear()
    line = {"case": "range"}
    line.update(figures("hip", hip), **figures("torch", tch))
    line.update(speedup_vs_torch=round(line["torch_ms"] / line["hip_ms"], 2), same_range=same, bytes_model=model,
                model_gbps=round(model / (line["hip_ms"] * 1e-3) / 1e9, 1),
                model_frac_hbm_peak=round(model / (line["hip_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4))
    emit(line)

    parts = [x[:rows // 10], x[rows // 10:]]
    for max_iter in (10, 40):
        hb = HomoBinning(max_iter=max_iter)
        hb.fit_split_points(parts)  # warm-up
        ts = []
        for _ in range(args.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hb.fit_split_points(parts)
            ts.append((time.perf_counter() - t0) * 1e3)
        emit({"case": "fit", "parties": 2, "bin_num": 10, "max_iter": max_iter, "passes": hb.last_report["passes"],
              "fixed": hb.last_report["fixed"], "fit_ms": round(statistics.median(ts), 2),
              "fit_ms_runs": [round(v, 2) for v in ts], "ms_per_pass": round(statistics.median(ts) /
                                                                             hb.last_report["passes"], 3),
              "timer": "host clock around the blocking call"})


if __name__ == "__main__":
    main()
