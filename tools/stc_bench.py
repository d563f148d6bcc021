#!/usr/bin/env python3
"""Sparse ternary compression on one GPU: kernels.stc (sfl_amd/csrc/sa_stc.hip)
against the torch restatement a user would write today (abs, a stable
torch.sort, scatter, mean, sign), on the same seeded data in one process.

Cases at --elems elements, rates 0.5 and 0.99:
* client: float32, u = (a - b) + r  -> sparse, res
* server: float64, u = a + r        -> sparse, res, acc += sparse

The two implementations alternate inside every pass (HIP events around
--reps / --torch-reps calls each, after a warm-up of both on the case's
shapes); a case's figure is the median over the passes of the per-pass
median.  One JSON line per case:

  hip_ms, torch_ms, speedup (torch_ms / hip_ms);
  bytes_moved: what the implementation's passes read and write (the model
    in DESIGN.md: form u, P - 1 further select passes, count, apply);
  bytes_min: read the operands once, write the results once;
  both over hip_ms as GB/s and as a fraction of the 8 TB/s HBM peak;
  same_support: the two implementations mask the same elements.

usage: python tools/stc_bench.py [--elems 100000000] [--reps 10] [--torch-reps 3] [--passes 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0
SELECT_PASSES = {4: 3, 8: 6}  # radix digits of a 31-bit / 63-bit key


def traffic(esz, has_b, has_r, has_acc, select):
    """(bytes moved, algorithmic minimum) per element."""
    ops = 1 + has_b + has_r
    form = ops * esz + esz                       # read the operands, write u
    hist = (SELECT_PASSES[esz] - 1) * esz if select else 0   # the first digit rides on the form pass
    count = esz                                  # ties per wave, survivors' sum
    apply_ = esz + 2 * esz + (2 * esz if has_acc else 0)      # read u; write sparse, res; acc both ways
    minimum = ops * esz + 2 * esz + (2 * esz if has_acc else 0)
    return form + hist + count + apply_, minimum


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("stc_bench: needs a GPU (no fallback)")
    dev = torch.device("cuda", 0)
    n = args.elems

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    lines = []
    for form, dtype in (("client", torch.float32), ("server", torch.float64)):
        g = torch.Generator(device=dev).manual_seed(7)
        a = torch.randn(n, generator=g, device=dev, dtype=dtype)
        b = a + torch.randn(n, generator=g, device=dev, dtype=dtype) * 1e-2 if form == "client" else None
        if form == "server":
            a.mul_(1e-2)
        r = torch.randn(n, generator=g, device=dev, dtype=dtype) * 1e-3
        acc = torch.randn(n, generator=g, device=dev, dtype=dtype) if form == "server" else None
        sparse, res = torch.empty_like(a), torch.empty_like(a)
        mu = torch.zeros(1, dtype=dtype, device=dev)
        scratch = torch.empty(K.stc_scratch_bytes(n, dtype), dtype=torch.uint8, device=dev)
        for rate in (0.5, 0.99):
            m = round(rate * n)
            keep = {}

            def hip():
                K.stc(a, b, r, m, sparse, res, acc=acc, mu_out=mu, scratch=scratch)

            def restatement():
                u = (a - b) + r if b is not None else a + r
                order = torch.sort(u.abs(), stable=True).indices
                um = u.clone()
                um[order[:m]] = 0
                mean = (um.abs().sum(dtype=torch.float64) / (n - m)).to(dtype)
                sp = mean * torch.sign(um)
                keep["sparse"], keep["res"] = sp, u - sp
                if acc is not None:
                    acc.add_(sp)

            hip(), restatement()  # warm-up of both on these shapes
            torch.cuda.synchronize()
            same = bool(torch.equal(sparse != 0, keep["sparse"] != 0))
            keep.clear()
            hs, ts = [], []
            for _ in range(args.passes):
                hs.append(timed(hip, args.reps))
                ts.append(timed(restatement, args.torch_reps))
                keep.clear()
            hip_ms, torch_ms = statistics.median(hs), statistics.median(ts)
            esz = a.element_size()
            moved, minimum = traffic(esz, b is not None, True, acc is not None, 0 < m < n)
            gbps = lambda per: per * n / (hip_ms * 1e-3) / 1e9  # noqa: E731
            lines.append({"case": f"{form}_{str(dtype).split('.')[-1]}_rate{rate}", "elems": n, "mask_num": m,
                          "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4),
                          "speedup": round(torch_ms / hip_ms, 2), "hip_ms_passes": [round(x, 4) for x in hs],
                          "torch_ms_passes": [round(x, 4) for x in ts],
                          "bytes_moved": moved * n, "bytes_min": minimum * n,
                          "moved_gbps": round(gbps(moved), 1), "moved_frac_hbm_peak": round(gbps(moved) / HBM_PEAK_GBPS, 3),
                          "min_gbps": round(gbps(minimum), 1), "min_frac_hbm_peak": round(gbps(minimum) / HBM_PEAK_GBPS, 3),
                          "launches": 4 + 2 * SELECT_PASSES[esz], "same_support": same,
                          "device": torch.cuda.get_device_name(0)})
            print(json.dumps(lines[-1]), flush=True)
        del a, b, r, acc, sparse, res
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
