#!/usr/bin/env python3
"""FedSMP's worker step on one GPU: the sa_smp kernels (sfl_amd/csrc/sa_smp.hip)
against the unfused three kernels and against the same arithmetic in torch ops
on a mask materialised by sa_smp_mask, on the same seeded data in one process.

Per keep ratio p (default 0.1 and 0.8) at --elems float32 elements, one JSON
line per case, device events, the implementations alternating inside every
pass (the figure is the median over the passes of the per-pass median):

* sumsq:    sa_smp_sumsq_f32 (reads old and new: 8 n bytes) beside
            sa_sumsq_f32 of a materialised d (4 n);
* perturb:  sa_smp_perturb_f32 (reads 8 n, writes 4 n) beside
            sa_dp_perturb_f32 of a materialised d (8 n);
* step:     both passes, against `unfused` (sa_smp_delta_f32, sa_sumsq_f32,
            sa_dp_perturb_f32, sa_smp_finish_f32: 36 n bytes) and `torch`
            (sub, mul, div, square().sum(float64), mul, randn noise add, mul,
            add on the materialised mask).

bytes_model over hip_ms gives GB/s and the fraction of benchkit/roofline's HBM
peak; DESIGN.md section 4 has sa_sumsq_f32 at 0.77 and sa_dp_perturb_f32 at
0.70 of it to read the fractions against.

usage: python tools/smp_bench.py [--elems 100000000] [--ratios 0.1,0.8] [--reps 10] [--passes 3] [--out FILE]
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
    ap.add_argument("--ratios", default="0.1,0.8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smp", "smp_bench.jsonl"))
    args = ap.parse_args()
    import torch

    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K
    from sfl_amd.security.privacy import SMPMask

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("smp_bench: needs a GPU (no fallback)")
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

    def ab(fns):
        """Per-pass medians of every implementation, alternating inside each pass."""
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        passes = {k: [] for k in fns}
        for _ in range(args.passes):
            for k, f in fns.items():
                passes[k].append(events(f, args.reps))
        return {k: statistics.median(v) for k, v in passes.items()}, passes

    lines = []

    def emit(case, p, med, passes, model, **extra):
        hip_ms = med["hip"]
        gbps = model / (hip_ms * 1e-3) / 1e9
        line = {"case": case, "ratio": p, "elems": n, "hip_ms": round(hip_ms, 4), "bytes_model": model,
                "model_gbps": round(gbps, 1), "model_frac_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4)}
        for k in med:
            if k != "hip":
                line[k + "_ms"] = round(med[k], 4)
                line["speedup_vs_" + k] = round(med[k] / hip_ms, 2)
        line["ms_passes"] = {k: [round(x, 4) for x in v] for k, v in passes.items()}
        line.update(extra, timer="device events", lib=os.path.basename(L.LIB_PATH),
                    device=torch.cuda.get_device_name(0))
        lines.append(line)
        print(json.dumps(line), flush=True)

    g = torch.Generator(device=dev).manual_seed(7)
    w0 = torch.randn(n, generator=g, device=dev) * 1e-1
    w1 = w0 + torch.randn(n, generator=g, device=dev) * 1e-3
    out, d, t = torch.empty_like(w0), torch.empty_like(w0), torch.empty_like(w0)
    part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    mbytes = torch.empty(n, dtype=torch.uint8, device=dev)
    sigma, updates, clip = 0.01, 8.0, 1.0
    for p in [float(v) for v in args.ratios.split(",")]:
        mask = SMPMask(0x0123456789ABCDEF, p)
        smp = mask.layer(0)
        c = float(mask.divisor)
        K.smp_sumsq(w0, w1, smp, total, part)
        dp = K.make_dp(total, l2_norm_clip=clip, noise_std=sigma, num_updates=updates, key=11, counter0=0)
        K.smp_mask(smp, mbytes)
        mf = mbytes.to(torch.float32)
        keep = {}

        def hip_sumsq():
            K.smp_sumsq(w0, w1, smp, total, part)

        def hip_perturb():
            K.smp_perturb(w0, w1, smp, dp, out)

        def hip_step():
            hip_sumsq()
            hip_perturb()

        def unfused():
            K.smp_delta(w0, w1, smp, d)
            K.sumsq_f32(d, total, part)
            K.dp_perturb(d, t, dp)
            K.smp_finish(w0, t, smp, out)

        def torch_step():
            dd = (w1 - w0).mul_(mf).div_(c)
            norm = dd.square().sum(dtype=torch.float64).sqrt()
            scale = torch.clamp(clip / norm, max=1.0).to(torch.float32)
            dd.mul_(scale).add_(torch.randn(n, device=dev).mul_(sigma / updates)).mul_(mf)
            keep["out"] = dd.add_(w0)

        K.smp_delta(w0, w1, smp, d)
        med, passes = ab({"hip": hip_sumsq, "plain": lambda: K.sumsq_f32(d, total, part)})
        emit("sumsq", p, med, passes, 8 * n, note="plain: sa_sumsq_f32 of a materialised d (4 n bytes)")
        med, passes = ab({"hip": hip_perturb, "plain": lambda: K.dp_perturb(d, t, dp)})
        emit("perturb", p, med, passes, 12 * n, note="plain: sa_dp_perturb_f32 of a materialised d (8 n bytes)")
        med, passes = ab({"hip": hip_step, "unfused": unfused, "torch": torch_step})
        fused_out = out.clone()
        unfused()
        emit("step", p, med, passes, 20 * n, unfused_bytes_model=36 * n,
             same_as_unfused=bool(torch.equal(fused_out.view(torch.int32), out.view(torch.int32))),
             kept_fraction=round(float(mf.mean(dtype=torch.float64)), 6))
        del mf, keep
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
