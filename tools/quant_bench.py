#!/usr/bin/env python3
"""The quantized compressors on one GPU: the sa_quant kernels
(sfl_amd/csrc/sa_quant.hip) against the same arithmetic written in torch ops
on the same device, on the same seeded data in one process.

Cases at --elems float32 elements for zero-point, LSTM and fp8 E4M3 at 8 bits,
and zero-point once on float64:
* compress:   range + code kernel with the scalars known (device events),
              against torch's aminmax / div / add / clamp / round / to(int8)
              (LSTM: mul / round / sub / clamp; fp8: abs / amax / mul / frexp /
              where / round / sign); `range_ms` and `code_ms` time the two
              passes apart; `class_ms` is `compress()` of the class with the
              host clock: it adds the pinned read of three words between them
* decompress: the decode kernel against to(float) / sub / mul (LSTM: add / div;
              fp8: abs / remainder / div / ldexp / sign)

The implementations alternate inside every pass (--reps / --torch-reps calls
each, after a warm-up of both on the case's shapes); a case's figure is the
median over the passes of the per-pass median, and the per-pass medians are
kept so the spread shows.  One JSON line per case:

  hip_ms, torch_ms, speedup (torch_ms / hip_ms);
  bytes_model: compress reads n s twice (range, codes) and writes n q;
    decompress reads n q and writes n s; over hip_ms as GB/s and as a fraction
    of benchkit/roofline's HBM peak;
  same: the two implementations gave the same bits;
  lib: the library timed (SFL_SA_LIB chooses another build, which is how
    profiles/quant/layout_ab.txt compared the lane layouts and grid bounds).

usage: python tools/quant_bench.py [--elems 100000000] [--reps 10] [--torch-reps 3] [--passes 3] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant", "quant_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K
    from sfl_amd.utils import quantized as Q

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("quant_bench: needs a GPU (no fallback)")
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

    def clock(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
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

    def emit(case, scheme, dtype, hip_ms, torch_ms, hs, ts, model, same, **extra):
        gbps = model / (hip_ms * 1e-3) / 1e9
        line = {"case": case, "scheme": scheme, "dtype": dtype, "elems": n, "hip_ms": round(hip_ms, 4),
                "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / hip_ms, 2),
                "hip_ms_passes": [round(x, 4) for x in hs], "torch_ms_passes": [round(x, 4) for x in ts],
                "bytes_model": model, "model_gbps": round(gbps, 1),
                "model_frac_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4), "same": same, "timer": "device events",
                "lib": os.path.basename(L.LIB_PATH), "device": torch.cuda.get_device_name(0)}
        line.update(extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    def scalar(v, like):
        """A 0-d device tensor: torch divides by a python scalar as a multiplication by its reciprocal."""
        return torch.zeros((), dtype=like.dtype, device=dev) + float(v)

    for scheme, tdt in (("zero_point", torch.float32), ("lstm", torch.float32), ("fp8_e4m3", torch.float32),
                        ("zero_point", torch.float64)):
        g = torch.Generator(device=dev).manual_seed(7)
        x = torch.randn(n, generator=g, device=dev, dtype=tdt) * 1e-2
        s = x.element_size()
        T = np.float32 if tdt == torch.float32 else np.float64
        comp = {"zero_point": Q.QuantizedZeroPoint, "lstm": Q.QuantizedLSTM, "fp8_e4m3": Q.QuantizedFP}[scheme]()
        c = comp.compress(x)
        codes = torch.empty(n, dtype=torch.int8, device=dev)
        out = torch.empty(n, dtype=tdt, device=dev)
        out3 = torch.empty(3, dtype=tdt, device=dev)
        scratch = torch.empty(K.quant_scratch_bytes(n, tdt), dtype=torch.uint8, device=dev)
        keep = {}

        def hip_range():
            K.quant_range(x, scratch, out3)

        if scheme == "zero_point":
            sc, z = scalar(c.scale, x), float(c.nudged_zero_point)

            def hip_code():
                K.quant_affine(x, L.SA_QUANT_ZERO_POINT, float(c.scale), z, -128, 127, codes)

            def torch_compress():
                keep["mm"] = torch.aminmax(x)
                keep["q"] = x.div(sc).add_(z).clamp_(-128, 127).round_().to(torch.int8)

            def hip_decompress():
                K.dequant_affine(codes, L.SA_QUANT_ZERO_POINT, float(c.scale), z, out)

            def torch_decompress():
                keep["d"] = codes.to(tdt).sub_(z).mul_(sc)
        elif scheme == "lstm":
            qq, rqm = scalar(c.q, x), float(T(c.rqm))

            def hip_code():
                K.quant_affine(x, L.SA_QUANT_LSTM, float(c.q), rqm, -128, 127, codes)

            def torch_compress():
                keep["mm"] = torch.aminmax(x)
                keep["q"] = x.mul(qq).round_().sub_(rqm).clamp_(-128, 127).to(torch.int8)

            def hip_decompress():
                K.dequant_affine(codes, L.SA_QUANT_LSTM, float(c.q), rqm, out)

            def torch_decompress():
                keep["d"] = codes.to(tdt).add_(rqm).div_(qq)
        else:
            sc = scalar(c.scale, x)
            ml, off = 8, 6

            def hip_code():
                K.quant_fp8(x, float(c.scale), ml, off, codes)

            def torch_compress():
                a = x.abs()
                keep["mm"] = a.amax()
                m, e = torch.frexp(a.mul_(sc))
                qe = torch.where(e > -off, e + off, 0)
                qm = m.mul_(2).sub_(1).mul_(ml).round_()
                keep["q"] = (torch.sign(x) * (qe * ml + qm)).to(torch.int8)

            def hip_decompress():
                K.dequant_fp8(codes, float(c.scale), ml, off, out)

            def torch_decompress():
                a = codes.to(torch.int32).abs_()
                mant = torch.remainder(a, ml).to(tdt).div_(ml).add_(1).div_(2)
                keep["d"] = (torch.sign(codes).to(tdt) * torch.ldexp(mant, a.div(ml, rounding_mode="floor") - off)
                             ).div_(sc)

        def hip_compress():
            hip_range()
            hip_code()

        label = "float32" if tdt == torch.float32 else "float64"
        hip_ms, torch_ms, hs, ts = ab(hip_compress, torch_compress)
        same = bool(torch.equal(codes, keep["q"]) and torch.equal(codes, c.compressed_data))
        range_ms, code_ms = events(hip_range, args.reps), events(hip_code, args.reps)
        class_ms = clock(lambda: comp.compress(x), args.reps)
        emit("compress", scheme, label, hip_ms, torch_ms, hs, ts, 2 * n * s + n, same, launches=3,
             range_ms=round(range_ms, 4), range_frac_hbm_peak=round(n * s / (range_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
             code_ms=round(code_ms, 4),
             code_frac_hbm_peak=round((n * s + n) / (code_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
             class_ms=round(class_ms, 4))
        keep.clear()
        hip_ms, torch_ms, hs, ts = ab(hip_decompress, torch_decompress)
        same = bool(torch.equal(out.view(torch.int32), keep["d"].view(torch.int32)))
        emit("decompress", scheme, label, hip_ms, torch_ms, hs, ts, n + n * s, same, launches=1)
        keep.clear()
        del x, codes, out, c
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
