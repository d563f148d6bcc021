#!/usr/bin/env python3
"""PPBAggregator's Paillier kernels on one GPU (sfl_amd/csrc/sa_ppb.hip):
encrypt (one party), add (--clients ciphertext arrays), decrypt, and the whole
``PPBAggregator.average`` of --clients float32 CUDA uploads, at K = 2048 and
K = 1024, for payloads of 37 x 1,024 and 1,000,000 elements a party (a fresh
key of each size is generated on the host first, outside every figure).

* hip:  the ``sa_ppb_*`` entry into device buffers, timed with device events:
        the median of --reps calls after one warm-up call; ``average`` is timed
        once a rep with a host clock around the call and a device
        synchronisation (it ends with a pinned read of the flag words).
* host: the package's host form (Python ``pow``) on one core of the same box,
        timed ONCE on --host-rows rows and SCALED to the payload's rows: an
        estimate, not a measurement of the whole payload.

One JSON line a (K, payload, case):

  rows, hip_ms, host_ms_scaled, speedup_vs_host (host / hip: below 1 is a loss);
  montmuls: Montgomery products a row by the kernel's schedule (the window
    table, five a window, the conversions), each counted at the ciphertext
    width of L = K / 16 limbs (decrypt's two products on K / 32 limbs are left
    out); montmul_per_s = rows montmuls / hip_ms;
  mul32_per_s = montmul_per_s * 2 L^2: the 32 x 32 -> 64 multiplies (one
    v_mad_u64_u32 each) that rate implies, L more a product for the quotient
    digits left out.

usage: python tools/ppb_bench.py [--clients 8] [--reps 3] [--host-rows 8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAYLOADS = (37 * 1024, 1_000_000)
KEY_BITS = (2048, 1024)
WINDOW = 4  # sa_ppb.h kWindow


def modexp_montmuls(ebits):
    """Products of sa_ppb.h's modexp: into Montgomery form, 14 table entries, five a window after the first."""
    return 1 + 14 + 5 * (-(-ebits // WINDOW) - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppb", "ppb_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from sfl_amd import _lib as L
    from sfl_amd import hostpipe as H
    from sfl_amd import kernels as K
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import ppb_aggregator as P

    L.lib()
    if not torch.cuda.is_available():
        raise SystemExit("ppb_bench: needs a GPU (no fallback)")
    dev = torch.device("cuda", 0)
    C = args.clients
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def events(fn):
        fn()  # warm-up
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), ts

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    server = PYU("server", 0)
    for bits in KEY_BITS:
        agg = P.PPBAggregator(server, [server] * C, paillier_key_size=bits)
        key, ln, limbs = agg.key, bits // 32, bits // 16
        public, private = agg._device_consts(dev, False), agg._device_consts(dev, True)
        # the host form's cost a row, once, on a few rows
        sample = [int.from_bytes(os.urandom(bits // 8), "little") % key.n for _ in range(args.host_rows)]
        t0 = time.perf_counter()
        cts = [key.encrypt(m, m | 1) for m in sample]
        host_enc = (time.perf_counter() - t0) / args.host_rows
        t0 = time.perf_counter()
        for a, b in zip(cts, cts[1:] + cts[:1]):
            for _ in range(C - 1):
                a = a * b % key.n2
        host_add = (time.perf_counter() - t0) / args.host_rows
        t0 = time.perf_counter()
        _ = [key.decrypt(c) for c in cts]
        host_dec = (time.perf_counter() - t0) / args.host_rows
        for n in PAYLOADS:
            rows = -(-n // agg.per_row)
            g = torch.Generator(device=dev).manual_seed(7)
            xs = [torch.randn(n, generator=g, device=dev) * 0.05 for _ in range(C)]
            flags = torch.zeros(1, dtype=K.LIMB, device=dev)
            plain = torch.empty(rows * ln, dtype=K.LIMB, device=dev)
            K.ppb_encode(xs[0], 1.0, float(C), C, agg.bias, agg.expand, bits, agg.len, plain, flags)
            ct = [torch.empty(rows * limbs, dtype=K.LIMB, device=dev) for _ in range(C)]
            total, back = torch.empty_like(ct[0]), torch.empty_like(plain)
            enc_ms, enc_all = events(lambda: K.ppb_encrypt(plain, rows, bits, public, agg.party_keys[0], 0, ct[0],
                                                           flags))
            for c in ct[1:]:
                c.copy_(ct[0])
            add_ms, add_all = events(lambda: K.ppb_add(ct, rows, bits, public, total))
            dec_ms, dec_all = events(lambda: K.ppb_decrypt(ct[0], rows, bits, private, total, back))
            assert np.array_equal(H.d2h(back, pooled=False), H.d2h(plain, pooled=False)), "decrypt(encrypt(m)) != m"
            uploads = [PYUObject(server, x) for x in xs]
            avg_all = []
            for _ in range(1 + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                agg.average(uploads, axis=0)
                torch.cuda.synchronize()
                avg_all.append((time.perf_counter() - t0) * 1e3)
            avg_ms = statistics.median(avg_all[1:])
            cases = {"encrypt": (enc_ms, enc_all, host_enc, modexp_montmuls(bits) + 2),
                     "add": (add_ms, add_all, host_add, 2 * (C - 1)),
                     "decrypt": (dec_ms, dec_all, host_dec, modexp_montmuls(key.lam.bit_length()) + 1),
                     "average": (avg_ms, avg_all[1:], C * host_enc + host_add + host_dec, None)}
            for case, (ms, every, host_row, mm) in cases.items():
                line = {"case": case, "key_bits": bits, "elements": n, "rows": rows, "clients": C,
                        "hip_ms": round(ms, 3), "hip_ms_reps": [round(t, 3) for t in every],
                        "host_ms_scaled": round(host_row * rows * 1e3, 1), "host_rows_timed": args.host_rows,
                        "speedup_vs_host": round(host_row * rows * 1e3 / ms, 1),
                        "timer": "perf_counter around the call" if case == "average" else "device events",
                        "device": torch.cuda.get_device_name(0)}
                if mm is not None:
                    rate = rows * mm / (ms * 1e-3)
                    line.update({"montmuls": mm, "limbs": limbs, "montmul_per_s": round(rate),
                                 "mul32_per_s": round(rate * 2 * limbs * limbs)})
                emit(line)


if __name__ == "__main__":
    main()
