#!/usr/bin/env python3
"""Instruction census of the fast-path tile loop of a k_clients instantiation
in the ISA file the Makefile keeps (hipcc -save-temps):

    python tools/loop_census.py [--json] [ISA.s] [XT CT L X K]

default: sfl_amd/lib/obj/sa_clients_f32-hip-amdgcn-amd-amdhsa-gfx950.s and
the 8-client sum-only launch, k_clients<float, float, 8, 0, 4> (f f 8 0 4).

A wave issues in order: every scalar instruction, scalar load and s_waitcnt
at its head is an issue turn in which it offers no VALU work, and at two
waves per SIMD the partner often cannot cover it.  The census counts that
scalar side of the loop beside its VALU instructions.

The tile loop is the loop (a label and a later branch back to it) that holds
the draws, i.e. the most v_mad_u64_u32 of inline-asm blocks (the prologue's
128-bit products are the compiler's own), the innermost such one; its fast
path is the walk
from the loop's label that falls through every conditional forward branch
(the compiler lays the likely side out as the fall-through: the exact
quantize path and the raw == 0 bookkeeping are branch targets), follows the
unconditional ones, and ends at the branch back to the label.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_ISA = os.path.join(ROOT, "sfl_amd", "lib", "obj", "sa_clients_f32-hip-amdgcn-amd-amdhsa-gfx950.s")
TYPES = {"f": "f", "float": "f", "d": "d", "double": "d", "x": "x", "i64": "x"}


def kernel_symbol(xt, ct, L, X, K):
    k = f"Li{K}E"
    return f"_ZN2sa9k_clientsI{TYPES[xt]}{TYPES[ct]}Li{L}ELi{X}E{k}EEvNS_5KArgsE"


def kernel_body(path, symbol):
    """The kernel's instruction / label lines, which of them stand in an
    inline-asm block, and its metadata counts."""
    body, in_asm, meta, inside, cur, asm = [], [], {}, False, None, False
    for line in open(path):
        s = line.strip()
        if s.split(";")[0].strip() == symbol + ":":
            inside = True
            continue
        if inside:
            if s.startswith(".Lfunc_end"):
                inside = False
                continue
            if s.startswith(";;#ASM"):
                asm = s.startswith(";;#ASMSTART")
            s = s.split(";")[0].strip()
            if s and not s.startswith((".", "#")) or re.match(r"\.LBB\d+_\d+:", s):
                body.append(s)
                in_asm.append(asm)
            continue
        m = re.match(r"\.name:\s+(\S+)", s)
        if m:
            cur = m.group(1)
        m = re.match(r"\.(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", s)
        if m:
            meta.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    return body, in_asm, meta.get(symbol, {})


def tile_loop(body, in_asm):
    """(index of the loop's label line, index of its back branch)."""
    labels = {s[:-1]: i for i, s in enumerate(body) if s.endswith(":")}
    best = None
    for j, s in enumerate(body):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)$", s)
        if not m or labels.get(m.group(1), j) >= j:
            continue
        i = labels[m.group(1)]
        mads = sum(1 for k in range(i, j) if in_asm[k] and body[k].startswith("v_mad_u64_u32"))
        key = (mads, -(j - i))
        if best is None or key > best[0]:
            best = (key, i, j)
    if best is None or best[0][0] == 0:
        raise SystemExit("no loop with draws (v_mad_u64_u32 in asm blocks) in this kernel")
    return best[1], best[2]


def fast_path(body, head, back):
    labels = {s[:-1]: i for i, s in enumerate(body) if s.endswith(":")}
    out, pc, seen = [], head, set()
    while True:
        if pc in seen or pc > back:
            raise SystemExit("the fast-path walk left the tile loop")
        seen.add(pc)
        s = body[pc]
        if s.endswith(":"):
            pc += 1
            continue
        out.append(s)
        m = re.match(r"(s_c?branch\S*)\s+(\.LBB\d+_\d+)$", s)
        if m:
            tgt = labels[m.group(2)]
            if tgt == head:
                return out
            if m.group(1) == "s_branch":
                pc = tgt
                continue
        pc += 1


CLASSES = ("s_load", "s_or_b64", "s_mov_b64", "s_waitcnt", "s_mov_b32")


def census(path=DEFAULT_ISA, xt="f", ct="f", L=8, X=0, K=4):
    symbol = kernel_symbol(xt, ct, L, X, K)
    body, in_asm, meta = kernel_body(path, symbol)
    if not body:
        raise SystemExit(f"{symbol} not found in {path}")
    head, back = tile_loop(body, in_asm)
    ins = fast_path(body, head, back)
    c = {"valu": 0, "scalar": 0, "vmem": 0, "lds": 0, "rest": 0, "mad_u64": 0}
    c.update({k: 0 for k in CLASSES})
    for s in ins:
        op = s.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
            c["mad_u64"] += op == "v_mad_u64_u32"
        elif op.startswith("s_"):
            c["scalar"] += 1
            for k in CLASSES:
                if op.startswith(k):
                    c[k] += 1
                    break
            else:
                c["rest"] += 1
        elif op.startswith(("buffer_", "global_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
    c["scratch"] = meta.get("private_segment_fixed_size", 0)
    c["vgpr"] = meta.get("vgpr_count")
    c["sgpr"] = meta.get("sgpr_count")
    c["sgpr_spill"] = meta.get("sgpr_spill_count", 0)
    c["vgpr_spill"] = meta.get("vgpr_spill_count", 0)
    c["kernel"] = symbol
    return c


def main():
    args = [a for a in sys.argv[1:] if a != "--json"]
    path = args.pop(0) if args and args[0].endswith(".s") else DEFAULT_ISA
    shape = args if args else ["f", "f", "8", "0", "4"]
    c = census(path, shape[0], shape[1], int(shape[2]), int(shape[3]), int(shape[4]))
    if "--json" in sys.argv:
        print(json.dumps(c))
        return
    pairs = c["mad_u64"] / 9  # draws: nine v_mad_u64_u32 each
    print(f"{c['kernel']}: fast-path tile loop, {c['mad_u64']} v_mad_u64_u32")
    print("| class | per tile |\n|---|---|")
    print(f"| VALU | {c['valu']:,} |")
    per = f" ({c['scalar'] / pairs:.1f} per pair draw)" if pairs else ""
    print(f"| scalar side, total | {c['scalar']}{per} |")
    for k, name in (("s_load", "`s_load_dword*`"), ("s_or_b64", "`s_or_b64` (zero test)"), ("s_mov_b64", "`s_mov_b64`"),
                    ("s_waitcnt", "`s_waitcnt`"), ("s_mov_b32", "`s_mov_b32`"), ("rest", "other scalar")):
        print(f"| {name} | {c[k]} |")
    print(f"| vector memory / LDS | {c['vmem']} / {c['lds']} |")
    print(f"| registers | {c['vgpr']} VGPRs, {c['sgpr']} SGPRs (as .sgpr_count), "
          f"{c['sgpr_spill']} SGPR / {c['vgpr_spill']} VGPR spills, {c['scratch']} B scratch |")


if __name__ == "__main__":
    main()
