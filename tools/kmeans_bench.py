#!/usr/bin/env python3
"""QuantizedKmeans on one GPU: the sa_kmeans kernels (sfl_amd/csrc/sa_kmeans.hip)
against the same Lloyd step written in torch ops on the same device, on the
same seeded data in one process; and, with --sklearn, the fit the reference
constructs (scikit-learn's ``KMeans(K, n_init=1, max_iter=50)``) on one core.

Cases at --elems elements: float32 at K = 8 and K = 256, float64 at K = 8.
* step:       one Lloyd step from the "cbrt" start (device events): the
              accumulate pass and the one-block update, the state reset before
              every call, against torch's ``bucketize`` / ``bincount`` /
              ``scatter_add_`` / integer division on the image ``u`` held as an
              int64 tensor (torch does not recompute the image: 8 bytes read
              per element where the kernel reads the tensor itself);
              ``same``: both give the same centres
* hist, labels, decode: the other three passes, timed alone
* class_ms:   ``compress()`` of the class with the host clock: the range, the
              histogram, ``max_iter`` = 50 steps enqueued back to back, the
              labels and the three pinned reads; ``n_iter`` is what the fit took
              (the steps after it return at once)

The implementations alternate inside every pass (--reps / --torch-reps calls
each, after a warm-up of both); a case's figure is the median over the passes
of the per-pass median, and the per-pass medians are kept so the spread shows.
One JSON line per case; ``bytes_model`` of a step is ``n * sizeof(T)`` read,
over ``hip_ms`` as GB/s and as a fraction of benchkit/roofline's HBM peak.

--sklearn times scikit-learn's fit on --sklearn-elems float32 normal values,
one thread (threadpoolctl), host clock, next to this project's numpy form and,
when there is a GPU, the device form on the same data; it needs no GPU.

usage: python tools/kmeans_bench.py [--elems 100000000] [--reps 10] [--torch-reps 3] [--passes 3] [--out FILE]
       python tools/kmeans_bench.py --sklearn [--sklearn-elems 4000000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("float32", 8), ("float32", 256), ("float64", 8))


def sklearn_lines(n, have_gpu):
    import numpy as np
    from sklearn.cluster import KMeans
    from threadpoolctl import threadpool_limits

    from sfl_amd.utils import quantized as Q

    x = np.random.default_rng(7).standard_normal(n).astype(np.float32)
    lines = []
    for K in (8, 256):
        with threadpool_limits(limits=1):
            t0 = time.perf_counter()
            km = KMeans(K, n_init=1, max_iter=50, random_state=0).fit(x.reshape(-1, 1))
            sk_s = time.perf_counter() - t0
        ours = Q.QuantizedKmeans(8, K, init="cbrt")
        t0 = time.perf_counter()
        c = ours.compress(x)
        np_s = time.perf_counter() - t0
        d = ours.decompress(c).astype(np.float64) - x
        line = {"case": "sklearn_baseline", "dtype": "float32", "elems": n, "k": K, "sklearn_one_core_s": round(sk_s, 3),
                "sklearn_n_iter": int(km.n_iter_), "numpy_form_s": round(np_s, 3), "n_iter": c.n_iter,
                "sse_ratio_ours_over_sklearn": round(float(np.dot(d, d)) / float(km.inertia_), 4),
                "timer": "host clock", "cpu": _cpu_name()}
        if have_gpu:
            import torch

            xd = torch.from_numpy(x).cuda()
            ours.compress(xd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ours.compress(xd)
            torch.cuda.synchronize()
            line["device_form_s"] = round(time.perf_counter() - t0, 5)
            line["device"] = torch.cuda.get_device_name(0)
        lines.append(line)
        print(json.dumps(line), flush=True)
    return lines


def _cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-elems", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans", "kmeans_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from sfl_amd import _lib as L

    L.lib()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.sklearn:
        lines = sklearn_lines(args.sklearn_elems, torch.cuda.is_available())
        with open(args.out, "a") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)
        return
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench: needs a GPU (no fallback)")
    from benchkit.roofline import HBM_PEAK_GBPS
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.utils import quantized as Q

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

    lines = []
    for label, k in CASES:
        tdt = torch.float32 if label == "float32" else torch.float64
        g = torch.Generator(device=dev).manual_seed(7)
        x = torch.randn(n, generator=g, device=dev, dtype=tdt) * 1e-2
        s_el = x.element_size()
        comp = Q.QuantizedKmeans(8, k, init="cbrt")
        mn, mx, _ = Q._range_device(x)
        mn, s, step = Q.kmeans_scale(mn, mx)
        hist = torch.empty(L.SA_KMEANS_BINS, dtype=torch.int32, device=dev)
        K.kmeans_hist(x, mn, s, hist)
        c0 = Q.kmeans_init(H.d2h(hist, pooled=False).view(np.uint32), k)
        words = np.zeros(L.SA_KMEANS_STATE_BYTES // 4, dtype=np.uint32)
        words[L.SA_KMEANS_STATE_C // 4:][:k] = c0
        state0 = H.h2d(words.view(np.uint8), dev)
        state = torch.empty_like(state0)
        codes = torch.empty(n, dtype=torch.int8, device=dev)
        out = torch.empty(n, dtype=tdt, device=dev)
        # the image for the torch form: int64 (torch has no uint32 arithmetic)
        u = torch.clamp(torch.round((x.to(torch.float64) - float(mn)) * float(s)), 0, float(Q.KMEANS_U)).to(torch.int64)
        cd = torch.from_numpy(c0.astype(np.int64)).to(dev)
        keep = {}

        def hip_step():
            state.copy_(state0)
            K.kmeans_step(x, mn, s, k, 1, state)

        def torch_step():
            b = (cd[:-1] + cd[1:]) >> 1
            lab = torch.bucketize(u, b, right=False)
            cnt = torch.bincount(lab, minlength=k)
            tot = torch.zeros(k, dtype=torch.int64, device=dev).scatter_add_(0, lab, u)
            one = cnt.clamp(min=1)
            quo, rem = torch.div(tot, one, rounding_mode="floor"), torch.remainder(tot, one)
            keep["c"] = torch.where(cnt > 0, quo + (2 * rem >= one).to(torch.int64), cd)

        hip_step(), torch_step()
        torch.cuda.synchronize()
        hs, ts = [], []
        for _ in range(args.passes):
            hs.append(events(hip_step, args.reps))
            ts.append(events(torch_step, args.torch_reps))
        hip_ms, torch_ms = statistics.median(hs), statistics.median(ts)
        got = H.d2h(state[L.SA_KMEANS_STATE_C:].view(torch.int32), pooled=False).view(np.uint32)[:k]
        same = bool(np.array_equal(got.astype(np.int64), keep["c"].cpu().numpy()))
        keep.clear()
        del u
        torch.cuda.empty_cache()
        hist_ms = events(lambda: K.kmeans_hist(x, mn, s, hist), args.reps)
        labels_ms = events(lambda: K.kmeans_labels(x, mn, s, k, state, 128, codes), args.reps)
        flag = K.coo_flag(dev)
        lut = H.h2d(Q.kmeans_centres(got.astype(np.uint64), mn, step, np.float32 if s_el == 4 else np.float64).reshape(-1),
                    dev)
        decode_ms = events(lambda: K.dequant_lut(codes, lut, 128, out, flag), args.reps)
        c = comp.compress(x)
        class_ms = clock(lambda: comp.compress(x), 3)
        gbps = n * s_el / (hip_ms * 1e-3) / 1e9
        line = {"case": "step", "dtype": label, "elems": n, "k": k, "hip_ms": round(hip_ms, 4),
                "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / hip_ms, 2),
                "hip_ms_passes": [round(v, 4) for v in hs], "torch_ms_passes": [round(v, 4) for v in ts],
                "bytes_model": n * s_el, "model_gbps": round(gbps, 1),
                "model_frac_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4), "same": same,
                "hist_ms": round(hist_ms, 4), "labels_ms": round(labels_ms, 4),
                "labels_frac_hbm_peak": round((n * s_el + n) / (labels_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                "decode_ms": round(decode_ms, 4),
                "decode_frac_hbm_peak": round((n * s_el + n) / (decode_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                "class_ms": round(class_ms, 3), "n_iter": c.n_iter, "max_iter": comp.max_iter,
                "timer": "device events", "lib": os.path.basename(L.LIB_PATH), "device": torch.cuda.get_device_name(0)}
        lines.append(line)
        print(json.dumps(line), flush=True)
        del x, codes, out, c
        torch.cuda.empty_cache()

    with open(args.out, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
