#!/usr/bin/env python3
"""MARS's feature pass on one GPU: the sa_mars kernels
(sfl_amd/csrc/sa_mars.hip) against ``torch.linalg.svdvals`` batched per layer
on the same device, and against the reference's per-channel ``np.linalg.svd``
loop on the host, for --clients clients of a ResNet-18-shaped layer list
(synthetic seeded weights, float32).

* hip:   one ``mars_sigma`` or ``mars_bn`` per plan entry into one features
         buffer (no read-back in the figure)
* torch: per conv / fc layer one ``svdvals`` of the stacked (clients x
         channels, C_in, kh kw) float32 batch, its first column times the
         BatchNorm scale in torch ops; the scale alone for a BatchNorm
* host:  the definition's loop (``mars_aggregator.features_host``: LAPACK per
         channel, float64) over host copies of the same weights, one client,
         scaled by --clients; timed once with a host clock (it takes seconds)

hip and torch alternate inside every pass (--reps / --torch-reps calls each, after a warm-up
of both on these shapes); a figure is the median over the passes of the
per-pass median, timed with device events.  One JSON line:

  hip_ms, torch_ms, host_ms; speedup_vs_torch, speedup_vs_host (other / hip:
    below 1 is not a gain);
  bytes_model: every conv, fc and BatchNorm weight and variance read once,
    the features written; that over hip_ms as GB/s and as a fraction of
    benchkit/roofline's HBM peak;
  matrices, launches; gram: which Gram form the library was built with
    (--gram, a label: the build decides);
  max_rel_vs_torch: the largest relative difference of a feature from the
    float32 torch value; max_ratio_vs_host: the largest |hip - host| over the
    tests' tolerance (K p / 2 + 64 p + 8) 2^-53 of client 0.

--wide measures sa_mars_sigma_wide instead (layers with a smaller side above
32: WIDE_SHAPES below), one JSON line per layer and one for all four:

* hip:   ``mars_sigma_wide`` per layer through one scratch tensor, as
         ``MarsAggregator(wide_layers="device")`` issues it (both kernels;
         their separate times come from a kernel trace of this command)
* torch: ``torch.linalg.matrix_norm(ord=2)`` of the stacked float32 batch
* host:  the parent's path for such a layer: ``hostpipe.d2h`` of every
         client's layer and ``mars_aggregator.entry_host`` (LAPACK per matrix,
         float64), all clients, timed once with a host clock, the copy included

usage: python tools/mars_bench.py [--clients 8] [--reps 10] [--torch-reps 2] [--passes 3] [--gram mfma] [--out FILE]
       python tools/mars_bench.py --wide [--clients 8] [--out profiles/mars/mars_wide_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resnet18_shapes(classes=10):
    """The parameter list of a ResNet-18 as MARS sees it: conv weights, groups of
    four BatchNorm vectors (weight, bias, mean, variance), the head."""
    shapes = [(64, 3, 7, 7)] + [(64,)] * 4
    cin = 64
    for cout, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        for block in range(2):
            shapes += [(cout, cin, 3, 3)] + [(cout,)] * 4 + [(cout, cout, 3, 3)] + [(cout,)] * 4
            if block == 0 and stride == 2:
                shapes += [(cout, cin, 1, 1)] + [(cout,)] * 4
            cin = cout
    return shapes + [(classes, 512), (classes,)]


WIDE_SHAPES = [(128, 784), (512, 512), (512, 4608), (128, 64, 7, 7)]


def wide(args):
    """The --wide mode (the module docstring)."""
    import numpy as np
    import torch

    from sfl_amd import _lib as L
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.security.aggregation import mars_aggregator as M

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("mars_bench: needs a GPU (no fallback)")
    dev = torch.device("cuda", 0)
    C = args.clients
    g = torch.Generator(device=dev).manual_seed(11)
    dims = [(s[0], s[1], s[2] * s[3]) if len(s) == 4 else (1,) + s for s in WIDE_SHAPES]
    ws = [[(torch.randn(s, generator=g, device=dev) * 0.05).reshape(-1) for _ in range(C)] for s in WIDE_SHAPES]
    stacked = [torch.stack(w).reshape((C * d[0],) + d[1:]) for w, d in zip(ws, dims)]
    offs = np.concatenate([[0], np.cumsum([C * d[0] for d in dims])]).astype(int)
    buf = torch.zeros(int(offs[-1]), dtype=torch.float64, device=dev)
    scratch = torch.empty(max(K.mars_wide_scratch_bytes(C, *d) for d in dims) // 8, dtype=torch.float64, device=dev)
    keep = {}

    def hip(which):
        for l in which:
            K.mars_sigma_wide(ws[l], *dims[l], scratch, buf, int(offs[l]))

    def torch_pass(which):
        keep["t"] = [torch.linalg.matrix_norm(stacked[l], ord=2) for l in which]

    def events(fn, which, reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(which)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    every = list(range(len(dims)))
    hip(every), torch_pass(every)  # warm-up of both on these shapes
    torch.cuda.synchronize()
    got = H.d2h(buf, pooled=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for which in [[l] for l in every] + [every]:
        hs, ts = [], []
        for _ in range(args.passes):
            hs.append(events(hip, which, args.reps))
            ts.append(events(torch_pass, which, args.torch_reps))
        hip_ms, torch_ms = statistics.median(hs), statistics.median(ts)
        host_ms, ratio = None, None
        if not args.skip_host:
            t0 = time.perf_counter()
            feats = [[M.entry_host({0: H.d2h(ws[l][i], pooled=False).reshape(WIDE_SHAPES[l])},
                                   [("conv" if dims[l][0] > 1 else "fc", 0)], 0) for i in range(C)] for l in which]
            host_ms = (time.perf_counter() - t0) * 1e3
            ratio = 0.0
            for l, f in zip(which, feats):
                p, k = min(dims[l][1:]), max(dims[l][1:])
                want = np.concatenate(f)
                mine = got[offs[l]:offs[l + 1]]
                ratio = max(ratio, float(np.max(np.abs(mine - want) / want)) / ((k * p / 2 + 64 * p + 8) * 2.0 ** -53))
        line = {"case": "wide", "layers": [list(WIDE_SHAPES[l]) for l in which], "dtype": "float32", "clients": C,
                "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4),
                "host_ms": None if host_ms is None else round(host_ms, 1),
                "speedup_vs_torch": round(torch_ms / hip_ms, 3),
                "speedup_vs_host": None if host_ms is None else round(host_ms / hip_ms, 2),
                "hip_ms_passes": [round(x, 4) for x in hs], "torch_ms_passes": [round(x, 4) for x in ts],
                "matrices": int(sum(C * dims[l][0] for l in which)), "max_ratio_vs_host": ratio,
                "timer": "device events; host: perf_counter, d2h included", "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--gram", default="mfma")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "mars", "mars_wide_bench.jsonl" if args.wide else "mars_bench.jsonl")
    if args.wide:
        return wide(args)
    import numpy as np
    import torch

    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import _lib as L
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.security.aggregation import mars_aggregator as M

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("mars_bench: needs a GPU (no fallback)")
    dev = torch.device("cuda", 0)
    C = args.clients
    shapes = resnet18_shapes()
    plan = M.clp_plan(shapes)
    g = torch.Generator(device=dev).manual_seed(11)
    models = []
    for _ in range(C):
        layers = [torch.randn(s, generator=g, device=dev) * (0.05 if len(s) > 1 else 1.0) for s in shapes]
        for kind, idx in plan:
            if kind == "bn":
                layers[idx + 3] = layers[idx + 3].abs() + 0.1
        models.append([x.contiguous() for x in layers])
    flat = [[m[l].reshape(-1) for m in models] for l in range(len(shapes))]
    sizes = [shapes[idx][0] if kind != "fc" else 1 for kind, idx in plan]
    offsets = np.concatenate([[0], np.cumsum([C * n for n in sizes])]).astype(int)
    buf = torch.zeros(int(offsets[-1]), dtype=torch.float64, device=dev)
    keep = {}

    def hip():
        for e, (kind, idx) in enumerate(plan):
            if kind == "bn":
                K.mars_bn(flat[idx], flat[idx + 3], buf, int(offsets[e]))
                continue
            s = shapes[idx]
            n_mat, rows, cols = (s[0], s[1], s[2] * s[3]) if kind == "conv" else (1, s[0], s[1])
            bn = M._bn_of(plan, e) if kind == "conv" else None
            K.mars_sigma(flat[idx], n_mat, rows, cols, buf, int(offsets[e]), bn_w=flat[bn] if bn is not None else (),
                         bn_var=flat[bn + 3] if bn is not None else ())

    def scale(idx):
        w, v = (torch.stack([m[idx + k] for m in models]) for k in (0, 3))
        return (w / torch.sqrt(v.clamp(min=0) + 1e-5)).abs()

    def torch_pass():
        outs = []
        for e, (kind, idx) in enumerate(plan):
            if kind == "bn":
                outs.append(scale(idx).reshape(-1))
                continue
            s = shapes[idx]
            w = torch.stack([m[idx] for m in models]).reshape((C * s[0], s[1], -1) if kind == "conv" else (C, s[0], s[1]))
            top = torch.linalg.svdvals(w)[:, 0]
            bn = M._bn_of(plan, e) if kind == "conv" else None
            outs.append(top * scale(bn).reshape(-1) if bn is not None else top)
        keep["t"] = torch.cat(outs)

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

    hip(), torch_pass()  # warm-up of both on these shapes
    torch.cuda.synchronize()
    hs, ts = [], []
    for _ in range(args.passes):
        hs.append(events(hip, args.reps))
        ts.append(events(torch_pass, args.torch_reps))
    hip_ms, torch_ms = statistics.median(hs), statistics.median(ts)
    got = H.d2h(buf, pooled=False)
    rel_torch = float(np.max(np.abs(got - H.d2h(keep["t"], pooled=False).astype(np.float64)) / got))

    host_ms, ratio = None, None
    if not args.skip_host:
        client0 = [H.d2h(x, pooled=False) for x in models[0]]
        t0 = time.perf_counter()
        feats = M.features_host(client0, plan)
        host_ms = (time.perf_counter() - t0) * 1e3 * C
        ratio = 0.0
        for e, (kind, idx) in enumerate(plan):
            if kind == "bn":
                continue
            s = shapes[idx]
            rows, cols = (s[1], s[2] * s[3]) if kind == "conv" else s
            tol = (max(rows, cols) * min(rows, cols) / 2 + 64 * min(rows, cols) + 8 + 4) * 2.0 ** -53
            mine = got[offsets[e]:offsets[e] + sizes[e]]
            ratio = max(ratio, float(np.max(np.abs(mine - feats[e]) / feats[e] / tol)))

    matrices = C * sum(n for n, (kind, _) in zip(sizes, plan) if kind != "bn")
    model = sum(C * int(np.prod(shapes[idx])) * 4 for kind, idx in plan if kind != "bn") \
        + sum(C * shapes[idx][0] * 4 * 2 for kind, idx in plan if kind == "bn") * 2 + int(offsets[-1]) * 8
    gbps = model / (hip_ms * 1e-3) / 1e9
    line = {"case": "features", "model": "resnet18-shaped", "dtype": "float32", "clients": C, "gram": args.gram,
            "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4),
            "host_ms": None if host_ms is None else round(host_ms, 1),
            "speedup_vs_torch": round(torch_ms / hip_ms, 2),
            "speedup_vs_host": None if host_ms is None else round(host_ms / hip_ms, 1),
            "hip_ms_passes": [round(x, 4) for x in hs], "torch_ms_passes": [round(x, 4) for x in ts],
            "matrices": matrices, "launches": len(plan), "features": int(offsets[-1]), "bytes_model": model,
            "model_gbps": round(gbps, 1), "model_frac_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4),
            "max_rel_vs_torch": rel_torch, "max_ratio_vs_host": ratio, "timer": "device events; host: perf_counter",
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
