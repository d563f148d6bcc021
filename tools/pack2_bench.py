#!/usr/bin/env python3
"""pack=2 against pack=1, not the headline bench: C clients x
--elems float32, device-resident, both forms in ONE process, alternating
window by window (a window: back-to-back steps between two HIP events, as
many as fill --window-ms of device time, at least --steps; --reps windows a
form after warm-up; the median window is reported with the spread).  Per form:

  step     the sum-only fused launch + the decode (what an aggregation runs)
  fused    the sum-only fused launch alone; roofline.frac by the bytes model
           (4*C*n + 8*n_words) / t against the 8 TB/s HBM peak
  party7   one party's launch with 7 streams and its wire image
  decode   the decode alone; bytes 8*n_words + 8*n

One JSON line each; ``speedup`` on a pack=2 line is pack=1's median over its
own.  usage: python tools/pack2_bench.py [--elems N] [--clients C] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", type=int, default=100_000_000)
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10, help="least steps of a window")
    ap.add_argument("--window-ms", type=float, default=120.0, help="device time a window should fill")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from oracle import secagg as o
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    L.lib()
    dev = torch.device("cuda", 0)
    C, n = args.clients, args.elems
    nw = (n + 1) // 2
    g = torch.Generator(device=dev).manual_seed(5)
    xs = [torch.randn(n, generator=g, device=dev) * 1e-2 for _ in range(C)]
    ws = [1.0] * C
    pg = [L.pcg64_from_seed(o.pair_seed(u, v)) for u in range(C) for v in range(u + 1, C)]
    ps = [1] * len(pg)
    party = [(L.pcg64_from_seed(o.pair_seed(0, v + 1)), 1, v) for v in range(7)]
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    s1 = torch.empty(n, dtype=K.U64, device=dev)
    s2 = s1[:nw]
    m1 = torch.empty(n, dtype=K.U64, device=dev)
    dec = torch.empty(n, dtype=torch.float64, device=dev)

    fused = {1: lambda: K.fused_clients(xs, ws, pg, ps, [], 0, s1, flags=flags),
             2: lambda: K.fused_clients_pack2(xs, ws, pg, ps, s2, flags=flags)}
    decode = {1: lambda: K.decode(s1, dec, divisor=float(C)),
              2: lambda: K.decode_pack2(s2, dec, divisor=float(C))}
    party7 = {1: lambda: K.mask(xs[0], m1, party, flags=flags),
              2: lambda: K.mask_pack2(xs[0], m1[:nw], party, C, flags=flags)}
    words = {1: n, 2: nw}
    cases = [("step", lambda p: (fused[p](), decode[p]()), lambda p: 4 * C * n + 16 * words[p] + 8 * n),
             ("fused", lambda p: fused[p](), lambda p: 4 * C * n + 8 * words[p]),
             ("party7", lambda p: party7[p](), lambda p: 4 * n + 8 * words[p]),
             ("decode", lambda p: decode[p](), lambda p: 8 * words[p] + 8 * n)]
    lines = []
    for name, run, nbytes in cases:
        times = {1: [], 2: []}
        steps = {1: args.steps, 2: args.steps}
        for rep in range(-args.warmup, args.reps):
            for p in (1, 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps[p]):
                    run(p)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1) / steps[p]
                if rep >= 0:
                    times[p].append(ms)
                elif rep == -args.warmup:  # the first warm-up window sizes the others
                    steps[p] = max(args.steps, int(args.window_ms / ms) + 1)
        assert int(flags.item()) == 0, "a launch flagged its inputs"
        med = {p: statistics.median(times[p]) for p in (1, 2)}
        for p in (1, 2):
            lines.append({"case": name, "pack": p, "clients": C, "elems": n, "ring_words": words[p],
                          "ms": round(med[p], 4), "ms_min": round(min(times[p]), 4), "ms_max": round(max(times[p]), 4),
                          "grad_elems_per_s": round((C if name in ("step", "fused") else 1) * n / med[p] * 1e3),
                          "bytes": nbytes(p),
                          "roofline": {"frac": round(nbytes(p) / med[p] / 1e6 / HBM_PEAK_GBPS, 4), "bound": "HBM bytes model"},
                          "speedup": round(med[1] / med[p], 3), "windows": args.reps, "steps_per_window": steps[p]})
    # the two forms decode the same values (pack=2's range rule holds for these inputs)
    fused[1](), decode[1]()
    ref = dec.clone()
    fused[2](), decode[2]()
    assert torch.equal(ref, dec), "pack=2 decoded differently from pack=1"
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
