#!/usr/bin/env python3
"""Top-k sparsification on one GPU: the sa_topk kernels
(sfl_amd/csrc/sa_topk.hip) against the torch composition a user would write on
the same device, on the same seeded data in one process.

Cases at --elems elements: float32 at sparse rates 0.9 and 0.99, float64 at 0.9.
* compress:   TopkSparse.compress (select + fill, outputs allocated inside)
              against abs + torch.topk + sort of the indices + gather
* kernels:    sa_topk_select + sa_topk_fill alone (outputs allocated before)
              against the same composition
* decompress: TopkSparse.decompress (memset, validated scatter, one pinned read
              of the flag) against zeros + index_put_
* mixed:      MixedCompressor(TopkSparse, QuantizedZeroPoint).compress end to
              end (float32 at 0.9 only; no torch counterpart)

The implementations alternate inside every pass (--reps / --torch-reps calls
each, after a warm-up of both on the case's shapes); a case's figure is the
median over the passes of the per-pass median.  compress and kernels are timed
with device events (nothing in them waits for the host); decompress and mixed
end in a blocking read and are timed with the host clock.  One JSON line per
case:

  hip_ms, torch_ms, speedup (torch_ms / hip_ms);
  bytes_model: the select reads x once per digit (3 for float32, 6 for
    float64), the count and the fill once each, and the fill writes
    k (4 + s): n s (digits + 2) + k (4 + s); decompress writes n s and reads
    k (4 + s);
  that over hip_ms as GB/s and as a fraction of benchkit/roofline's HBM peak;
  same: both implementations selected the same set (and gave the same bits);
  differ / differ_only_in_ties: the positions only one of them kept, and whether
    all of those hold the threshold magnitude, where torch.topk breaks ties
    its own way.

usage: python tools/topk_bench.py [--elems 100000000] [--reps 10] [--torch-reps 2] [--passes 3] [--out FILE]
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
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "topk_bench.jsonl"))
    args = ap.parse_args()
    import torch

    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import _lib as L
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.utils import compressor as C
    from sfl_amd.utils.sparse_compressor import keep_count

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench: needs a GPU (no fallback)")
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

    def ab(hip, other, timer):
        hip(), other()  # warm-up of both on these shapes
        torch.cuda.synchronize()
        hs, ts = [], []
        for _ in range(args.passes):
            hs.append(timer(hip, args.reps))
            ts.append(timer(other, args.torch_reps))
        return statistics.median(hs), statistics.median(ts), hs, ts

    lines = []

    def emit(case, dtype, rate, k, hip_ms, torch_ms, hs, ts, model, same, timer, **extra):
        gbps = model / (hip_ms * 1e-3) / 1e9
        line = {"case": case, "elems": n, "dtype": dtype, "sparse_rate": rate, "k": k, "hip_ms": round(hip_ms, 4),
                "torch_ms": None if torch_ms is None else round(torch_ms, 4),
                "speedup": None if torch_ms is None else round(torch_ms / hip_ms, 2),
                "hip_ms_passes": [round(x, 4) for x in hs], "torch_ms_passes": [round(x, 4) for x in ts],
                "bytes_model": model, "model_gbps": round(gbps, 1),
                "model_frac_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4), "same": same, "timer": timer,
                "device": torch.cuda.get_device_name(0)}
        line.update(extra)
        lines.append(line)
        print(json.dumps(line), flush=True)

    bits = {torch.float32: torch.int32, torch.float64: torch.int64}
    for tdt, rate in ((torch.float32, 0.9), (torch.float32, 0.99), (torch.float64, 0.9)):
        g = torch.Generator(device=dev).manual_seed(7)
        x = torch.randn(n, generator=g, device=dev, dtype=tdt)
        s, digits = x.element_size(), 3 if tdt == torch.float32 else 6
        k = keep_count(rate, n)
        name = str(tdt).replace("torch.", "")
        comp = C.TopkSparse(rate)
        keep = {}

        def hip_compress():
            keep["c"] = comp.compress(x)

        def torch_compress():
            idx = torch.sort(torch.topk(x.abs(), k, sorted=False).indices).values
            keep["t"] = (idx, x[idx])

        def same_as_torch(index, data):
            return bool(torch.equal(index.to(torch.int64), keep["t"][0])
                        and torch.equal(data.view(bits[tdt]), keep["t"][1].view(bits[tdt])))

        def ties_of(index, data):
            """Where the two sets differ: how many positions each has alone, and
            whether every one of them holds the threshold magnitude (torch.topk
            breaks such ties its own way; 10^8 float32 normals have several
            elements per representable value around the threshold)."""
            mine, theirs = index.to(torch.int64), keep["t"][0]
            only_mine = mine[~torch.isin(mine, theirs)]
            only_theirs = theirs[~torch.isin(theirs, mine)]
            tau = data.abs().min()
            ties = bool(only_mine.numel() == only_theirs.numel() and (x[only_mine].abs() == tau).all()
                        and (x[only_theirs].abs() == tau).all())
            return {"differ": int(only_mine.numel()), "differ_only_in_ties": ties}

        model = n * s * (digits + 2) + k * (4 + s)
        hip_ms, torch_ms, hs, ts = ab(hip_compress, torch_compress, events)
        c = keep["c"]
        emit("compress", name, rate, k, hip_ms, torch_ms, hs, ts, model, same_as_torch(c.index, c.compressed_data),
             "device events", launches=2 * digits + 4, **ties_of(c.index, c.compressed_data))

        scratch = torch.empty(K.topk_scratch_bytes(n, tdt), dtype=torch.uint8, device=dev)
        index, data, flag = torch.empty_like(c.index), torch.empty_like(c.compressed_data), K.coo_flag(dev)
        parts = {}

        def hip_kernels():
            K.topk_select(x, k, scratch)
            K.topk_fill(x, x, k, scratch, index, data, flag)

        hip_ms, torch_ms, hs, ts = ab(hip_kernels, torch_compress, events)
        same = same_as_torch(index, data) and H.d2h(flag, pooled=False).tolist() == [0, -1]
        parts["select_ms"] = round(events(lambda: K.topk_select(x, k, scratch), args.reps), 4)
        parts["fill_ms"] = round(events(lambda: K.topk_fill(x, x, k, scratch, index, data, flag), args.reps), 4)
        emit("kernels", name, rate, k, hip_ms, torch_ms, hs, ts, model, same, "device events",
             launches=2 * digits + 4, **parts, **ties_of(index, data))
        del index, data

        long_index = c.index.to(torch.int64)  # index_put_ wants int64: converted outside the timed call

        def hip_decompress():
            keep["h"] = comp.decompress(c)

        def torch_decompress():
            keep["d"] = torch.zeros(n, dtype=tdt, device=dev).index_put_((long_index,), c.compressed_data)

        hip_ms, torch_ms, hs, ts = ab(hip_decompress, torch_decompress, clock)
        same = bool(torch.equal(keep["h"].view(bits[tdt]), keep["d"].view(bits[tdt])))
        emit("decompress", name, rate, k, hip_ms, torch_ms, hs, ts, n * s + k * (4 + s), same, "host clock",
             launches=2)
        keep.clear()
        del long_index

        if tdt == torch.float32 and rate == 0.9:
            mixed = C.MixedCompressor(C.TopkSparse(rate), C.QuantizedZeroPoint())

            def hip_mixed():
                keep["m"] = mixed.compress(x)

            hip_mixed()
            hs = [clock(hip_mixed, args.reps) for _ in range(args.passes)]
            m = keep["m"]
            back = mixed.decompress(m)
            kept = back != 0
            err = float((back[kept] - x[kept]).abs().max())
            emit("mixed_zero_point", name, rate, k, statistics.median(hs), None, hs, [],
                 model + k * s + k * (s + 1), bool(torch.equal(m.compressed_participants[0].index, c.index)),
                 "host clock", payload_bytes=m.nbytes, max_abs_error=round(err, 6),
                 scale=float(m.compressed_participants[1].scale))
            keep.clear()
        del x, c
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
