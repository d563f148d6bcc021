#!/usr/bin/env python3
"""FeatureHistogram on one GPU: the sa_hist kernels (sfl_amd/csrc/sa_hist.hip)
against the same result from torch ops on the same device, on the same seeded
data in one process.

Cases: float32, --rows x 64 features at 64 and at 255 split points a feature,
batches of 1, 8 and 20 nodes (every row in a node, drawn uniformly).
* codes:  the codes pass alone (device events) against ``torch.bucketize`` a
          feature
* hist:   build + finish (device events) against torch's ``scatter_add_`` of
          the float64 gradients and ``bincount`` into (node, feature, code),
          then ``cumsum``; ``same_counts`` / ``max_rel_diff``: the two results
          agree (torch's sums are float64 in atomic order, ours are exact in
          fixed point, so the sums agree to rounding only)
* ref:    the reference's definition (a masked sum per split point) in numpy on
          one host core at --ref-rows rows, scaled linearly to --rows and
          labelled as scaled

The implementations alternate inside every pass (--reps / --torch-reps calls
each, after a warm-up of both); a figure is the median over the passes of the
per-pass median, and the per-pass medians are kept.  ``bytes_model``: codes,
node_of_row, grad and hess read once per feature group and launch; its
GB/s over benchkit/roofline's HBM peak is ``model_frac_hbm_peak``.

usage: python tools/hist_bench.py [--rows 10000000] [--reps 5] [--torch-reps 2] [--passes 3] [--out FILE]
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
BINS = (64, 255)
NODES = (1, 8, 20)


def reference_seconds(rows, bins):
    """The reference's loops (feature_histogram.py: a masked sum per split
    point) on one core, one node, ``rows`` rows."""
    import numpy as np

    rng = np.random.default_rng(7)
    data = rng.standard_normal((rows, 3))
    pts = np.sort(rng.standard_normal(bins))
    t0 = time.perf_counter()
    for _ in range(F):
        for t in pts:
            m = data[data[:, 0] < t]
            m.sum(axis=0), m.shape[0]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--ref-rows", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist", "hist_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from sfl_amd import _lib as L

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("hist_bench: needs a GPU (no fallback)")
    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.ml.boost import FeatureHistogram

    dev = torch.device("cuda", 0)
    rows = args.rows
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

    def alternate(ours, theirs):
        ours(), theirs()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.passes):
            a.append(events(ours, args.reps))
            b.append(events(theirs, args.torch_reps))
        return a, b

    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn((rows, F), generator=g, device=dev, dtype=torch.float32)
    grad = torch.randn(rows, generator=g, device=dev, dtype=torch.float32)
    hess = torch.rand(rows, generator=g, device=dev, dtype=torch.float32)
    lines = []
    for bins in BINS:
        rng = np.random.default_rng(bins)
        splits = [np.sort(rng.standard_normal(bins).astype(np.float32)).astype(np.float64) for _ in range(F)]
        fh = FeatureHistogram(splits)
        fh.set_gradients(grad, hess)
        sd = [H.h2d(s.astype(np.float32), dev) for s in splits]
        keep = {}

        def hip_codes():
            keep["codes"] = fh.bind(x)

        def torch_codes():
            keep["tcodes"] = torch.stack([torch.bucketize(x[:, f], sd[f], right=True) for f in range(F)], dim=1)

        hc, tc = alternate(hip_codes, torch_codes)
        codes = keep["codes"]
        same_codes = bool((codes == keep["tcodes"]).all())  # float32 split points on both sides
        keep.clear()
        codes_ms, tcodes_ms = statistics.median(hc), statistics.median(tc)
        line = {"case": "codes", "dtype": "float32", "rows": rows, "features": F, "bins": bins,
                "hip_ms": round(codes_ms, 4), "torch_ms": round(tcodes_ms, 4), "speedup": round(tcodes_ms / codes_ms, 2),
                "hip_ms_passes": [round(v, 4) for v in hc], "torch_ms_passes": [round(v, 4) for v in tc],
                "bytes_model": rows * F * 5, "same_codes": same_codes,
                "model_frac_hbm_peak": round(rows * F * 5 / (codes_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                "timer": "device events", "device": torch.cuda.get_device_name(0)}
        lines.append(line)
        print(json.dumps(line), flush=True)
        ref_s = reference_seconds(args.ref_rows, bins)
        ncodes = bins + 1
        for n_nodes in NODES:
            node = torch.randint(0, n_nodes, (rows,), generator=g, device=dev, dtype=torch.int32)
            fbase = torch.arange(F, device=dev, dtype=torch.int64) * ncodes

            def hip_hist():
                keep["out"] = fh.calculate_histogram(codes, node, n_nodes)

            def torch_hist():
                idx = ((node.to(torch.int64) * (F * ncodes))[:, None] + fbase[None, :] + codes).reshape(-1)
                size = n_nodes * F * ncodes
                cols = [torch.zeros(size, dtype=torch.float64, device=dev).scatter_add_(
                    0, idx, v.to(torch.float64)[:, None].expand(rows, F).reshape(-1)) for v in (grad, hess)]
                cols.append(torch.bincount(idx, minlength=size).to(torch.float64))
                keep["tout"] = torch.cumsum(torch.stack(cols, dim=1).view(n_nodes, F, ncodes, 3), dim=2)[:, :, :bins]

            hh, th = alternate(hip_hist, torch_hist)
            ours, theirs = keep["out"], keep["tout"]
            same_counts = bool((ours[..., 2] == theirs[..., 2]).all())
            scale = theirs[..., :2].abs().amax().clamp(min=1e-300)
            rel = H.d2h(((ours[..., :2] - theirs[..., :2]).abs().amax() / scale).reshape(1), pooled=False)[0]
            keep.clear()
            hip_ms, torch_ms = statistics.median(hh), statistics.median(th)
            fg, slots, launches, lds = K.hist_geometry(bins, n_nodes, F)
            model = launches * ((F + fg - 1) // fg) * rows * (fg + 12)
            line = {"case": "hist", "dtype": "float32", "rows": rows, "features": F, "bins": bins, "nodes": n_nodes,
                    "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / hip_ms, 2),
                    "hip_ms_passes": [round(v, 4) for v in hh], "torch_ms_passes": [round(v, 4) for v in th],
                    "feature_group": fg, "slots_per_launch": slots, "launches": launches, "lds_bytes": lds,
                    "bytes_model": model, "model_gbps": round(model / (hip_ms * 1e-3) / 1e9, 1),
                    "model_frac_hbm_peak": round(model / (hip_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                    "lds_atomics_per_ns": round(3 * rows * F / (hip_ms * 1e6), 2),
                    "same_counts": same_counts, "max_rel_diff": float(rel),
                    "reference_one_core_s_scaled": round(ref_s * rows / args.ref_rows, 1),
                    "reference_note": f"scaled: measured {round(ref_s, 3)} s at {args.ref_rows} rows, one node, times "
                                      "rows / ref_rows (the masked sums are linear in the rows)",
                    "timer": "device events", "lib": os.path.basename(L.LIB_PATH),
                    "device": torch.cuda.get_device_name(0)}
            lines.append(line)
            print(json.dumps(line), flush=True)
            with open(args.out, "w") as f:
                f.writelines(json.dumps(ln) + "\n" for ln in lines)
            del node, ours, theirs
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
