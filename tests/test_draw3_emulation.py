"""The three-carry PCG64 draw (sfl_amd/csrc/sa_draw3.h, which the build writes
with tools/gen_draw2.py --carry3), executed on the CPU against Python integers.

The form drops the carry out of the step's weight-2^32 column
O1 = s0*a1 + c1 + s1*a0, which is exact only while O1 < 2^64, i.e. for a
multiplier whose low limbs satisfy a0 + a1 + 1 <= 2^32 (pcg128.h,
carry_free).  Every block of the header -- ss, sa, as, aa, one, one_same,
every first-touch set -- runs on test_draw_emulation.py's gfx950 interpreter
with PCG64's own multiplier and with the tile jump's A^(g*512 - 1) of
qualifying grids, on states that include O1's maximum (s0 = s1 = c1 =
0xFFFFFFFF), and is compared with (S*M + C) mod 2^128, the XSL-RR output, the
accumulators and the zero mask.  A control shows those inputs decide: with a
non-qualifying multiplier (grid 511's) the same block leaves a wrong state.
The header's text is pinned to the generator, to its instruction counts and
to the VALU-written-SGPR read distance."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_draw_asm import CARRY, _sgpr_operands
from test_draw_emulation import Lane, _functions, _raw, _states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sfl_amd", "csrc", "sa_draw3.h")
GEN = os.path.join(ROOT, "tools", "gen_draw2.py")
M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1
A = 0x2360ED051FC65DA44385DF649FCCF645
GRIDS = (2, 8, 508, 512, 1024)  # qualifying grids: the tile jump is A^(g*512 - 1)
NAMES = ["pcg_draw2_pair_ss", "pcg_draw2_pair_sa", "pcg_draw2_pair_as", "pcg_draw2_pair_aa",
         "pcg_draw2_one", "pcg_draw2_one_same"]


def _jump_mult(grid):
    return pow(A, grid * 512 - 1, 1 << 128)


def _carry_free(mult):
    return (mult & M32) + ((mult >> 32) & M32) + 1 <= 1 << 32


MULTS = [("A", A)] + [(f"grid{g}", _jump_mult(g)) for g in GRIDS]


_TEXT = []


def _header_text():
    """What the generator emits: the header's text, with or without a build."""
    if not _TEXT:
        _TEXT.append(subprocess.run([sys.executable, GEN, "--carry3"], capture_output=True, text=True,
                                    check=True).stdout)
    return _TEXT[0]


def _funcs():
    return _functions(_header_text())


def _cases(mult, rng):
    """(state before the step, increment) pairs: _states()'s rotations (r = 0,
    small, large, a raw 0, random), moved to this multiplier -- the same next
    states, reached by `mult` -- and the states that decide the dropped carry."""
    minv = pow(mult, -1, 1 << 128)
    out = []
    for s, inc in _states(rng):
        nxt = (s * A + inc) & M128
        out.append(((nxt - inc) * minv & M128, inc))
    assert _raw((out[3][0] * mult + out[3][1]) & M128) == 0  # the state that draws raw 0
    hi = int(rng.integers(0, 1 << 62)) << 64
    inc_max = (int(rng.integers(0, 1 << 62)) << 64 | M32 << 32 | int(rng.integers(0, 1 << 31)) * 2 + 1) & M128
    inc = (int(rng.integers(0, 1 << 62)) << 64 | int(rng.integers(0, 1 << 62))) | 1
    out.append((hi | M64, inc_max))    # s0 = s1 = c1 = 0xFFFFFFFF: O1's maximum
    out.append((hi | M32, inc))        # s0 = 0xFFFFFFFF, s1 = 0
    out.append((hi | M32 << 32, inc))  # s0 = 0, s1 = 0xFFFFFFFF
    return out


def _run(lines, mult, sa, sb, ma, mb, acc, bias, rng):
    """One block on one lane; returns (env, next states)."""
    env = {f"a{i}": (mult >> (32 * i)) & M32 for i in range(4)}
    env.update({"ma": ma, "mb": mb, "mma": ma << 32 | ma, "mmb": mb << 32 | mb, "zh": 0})
    for t, (s, inc) in (("a", sa), ("b", sb)):
        env[f"p01{t}"] = s & M64
        env[f"s2{t}"] = (s >> 64) & M32
        env[f"s3{t}"] = s >> 96
        env[f"c0{t}"] = inc & M32
        env[f"c1{t}"] = (inc >> 32) & M32
        env[f"c23{t}"] = inc >> 64
    env.update(acc)
    env.update({"b" + k: v for k, v in bias.items()})
    for k in ("va", "vb"):  # the subtracting partners' halves
        env[k + "lo"], env[k + "hi"] = acc[k] & M32, acc[k] >> 32
    lane = Lane(env, rng)
    for line in lines:
        lane.run(line)
    got = {t: lane.env[f"p01{t}"] | lane.env[f"s2{t}"] << 64 | lane.env[f"s3{t}"] << 96 for t in "ab"}
    return lane.env, got


def _check_block(name, F, lines, mult, sa, sb, ma, mb, rng):
    acc = {k: int(rng.integers(0, 1 << 63)) * 2 + 1 for k in ("ua", "va", "ub", "vb")}
    bias = {k: int(rng.integers(0, 1 << 63)) * 2 + 1 for k in ("ua", "va", "ub", "vb")}
    env, got = _run(lines, mult, sa, sb, ma, mb, acc, bias, rng)
    t, zero = {}, False
    for tag, (s, inc), m in (("a", sa, ma), ("b", sb, mb)):
        nxt = (s * mult + inc) & M128
        assert got[tag] == nxt, (name, F, tag, hex(s))
        raw = _raw(nxt)
        zero |= raw == 0
        t[tag] = raw ^ (M64 if m else 0)
    assert (env["zh"] != 0) == zero, (name, F)
    # a first-touched accumulator starts from its client's bias, not its old value
    start = {k: bias[k] if F & bit else acc[k] for k, bit in (("ua", 1), ("va", 2), ("ub", 4), ("vb", 8))}
    if name.endswith("one_same"):  # both cross streams of one client
        assert env["ua"] == (start["ua"] + t["a"] + t["b"]) & M64, (name, F)
        return
    assert env["ua"] == (start["ua"] + t["a"]) & M64, (name, F)
    assert env["ub"] == (start["ub"] + t["b"]) & M64, (name, F)
    if "pair" in name:
        for tag, mode in zip("ab", name[-2:]):
            k = "v" + tag
            if mode == "a":
                assert env[k] == (start[k] + t[tag]) & M64, (name, F, tag)
            else:
                assert env[k + "lo"] | env[k + "hi"] << 32 == (acc[k] - t[tag]) & M64, (name, F, tag)


@pytest.mark.parametrize("mname,mult", MULTS, ids=[m[0] for m in MULTS])
@pytest.mark.parametrize("name", NAMES)
def test_every_block_equals_python_integers(name, mname, mult):
    assert _carry_free(mult), mname
    blocks = _funcs()[name]
    assert blocks, name
    rng = np.random.default_rng(sum(map(ord, name + mname)))
    cases = _cases(mult, rng)
    checked = 0
    for F, lines in sorted(blocks.items()):
        for i, sa in enumerate(cases):
            sb = cases[(i + 3) % len(cases)]
            for ma, mb in ((0, 0), (M32, 0), (0, M32), (M32, M32)):
                _check_block(name, F, lines, mult, sa, sb, ma, mb, rng)
                checked += 1
    assert checked == len(blocks) * len(cases) * 4 and len(cases) == 9


def test_first_touch_sets_are_all_there():
    sets = {n: sorted(b) for n, b in _funcs().items()}
    assert sets == {"pcg_draw2_pair_ss": [0, 1, 4, 5], "pcg_draw2_pair_sa": [0, 1, 4, 5, 8, 9, 12, 13],
                    "pcg_draw2_pair_as": list(range(8)), "pcg_draw2_pair_aa": list(range(16)),
                    "pcg_draw2_one": [0, 1, 4, 5], "pcg_draw2_one_same": [0, 1]}


@pytest.mark.parametrize("name", NAMES)
def test_control_a_non_qualifying_multiplier_breaks_the_all_ones_state(name):
    """Grid 511's tile jump has a0 + a1 + 1 = 0x114B91EAE > 2^32: with
    s0 = s1 = c1 = 0xFFFFFFFF the middle column overflows 64 bits and the
    three-carry block, which drops that carry, must leave a state that differs
    from (S*M + C) mod 2^128.  (A CPU emulation of a constant no launch uses:
    launch_clients refuses it.)  The general form, sa_draw2.h, stays exact."""
    mult = _jump_mult(511)
    assert (mult & M32) + ((mult >> 32) & M32) + 1 == 0x114B91EAE and not _carry_free(mult)
    rng = np.random.default_rng(511)
    s, inc = _cases(mult, rng)[6]
    assert s & M64 == M64 and (inc >> 32) & M32 == M32
    want = (s * mult + inc) & M128
    acc = {k: 1 for k in ("ua", "va", "ub", "vb")}
    _, got = _run(_funcs()[name][0], mult, (s, inc), (s, inc), 0, 0, acc, acc, rng)
    assert got["a"] != want and got["b"] != want
    assert (got["a"] ^ want) & ((1 << 96) - 1) == 0  # limbs 0-2 are right: the lost carry belongs to limb 3
    general = _functions(open(os.path.join(ROOT, "sfl_amd", "csrc", "sa_draw2.h")).read())
    _, got4 = _run(general[name][0], mult, (s, inc), (s, inc), 0, 0, acc, acc, rng)
    assert got4["a"] == want and got4["b"] == want


def test_header_matches_generator_and_budget():
    text = _header_text()
    assert os.path.exists(HEADER), "the build writes sa_draw3.h (sfl_amd/csrc/Makefile); run __graft_entry__.build()"
    assert open(HEADER).read() == text, "sa_draw3.h is stale: the Makefile rebuilds it from tools/gen_draw2.py"
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "sfl_amd/csrc/sa_draw3.h" in ignored  # generated, kept out of git
    assert '#define SA_DRAW2_FORM "rots_carry3"' in text and '"s_nop' not in text
    counts = dict(re.findall(r"// (pcg_draw2_\w+): (\d+) VALU \+ 0 s_nop", text))
    assert {k: int(v) for k, v in counts.items()} == {
        "pcg_draw2_pair_ss": 48, "pcg_draw2_pair_sa": 47, "pcg_draw2_pair_as": 47, "pcg_draw2_pair_aa": 46,
        "pcg_draw2_one": 44, "pcg_draw2_one_same": 44}
    # counted on the blocks themselves, not only read from the comments
    for name, blocks in _funcs().items():
        for lines in blocks.values():
            assert sum(ln.startswith("v_") for ln in lines) == int(counts[name]), name
            assert sum("v_addc_co_u32" in ln for ln in lines) == 4  # two joins with a carry-in per draw
            assert sum("v_mad_u64_u32" in ln for ln in lines) == 18


def test_default_generator_output_is_still_the_general_form():
    gen = subprocess.run([sys.executable, GEN], capture_output=True, text=True, check=True).stdout
    assert gen == open(os.path.join(ROOT, "sfl_amd", "csrc", "sa_draw2.h")).read()
    assert '#include "sa_draw3.h"' in open(os.path.join(ROOT, "sfl_amd", "csrc", "sa_clients_impl.h")).read()


def test_valu_sgpr_write_read_distance_of_the_new_header():
    """test_draw_asm.py's scan on sa_draw3.h: an SGPR written by a VALU
    instruction (a carry-out, a compare mask) is read no earlier than the
    third instruction after the write -- with no s_nop to make room."""
    checked = 0
    for name, blocks in _funcs().items():
        for blk in blocks.values():
            last_write = {}
            for i, ins in enumerate(blk):
                op, _, args = ins.partition(" ")
                parts = [p.strip() for p in re.split(r",(?![^\[]*\])", args)]
                writes, reads = set(), set()
                if op.startswith("v_cmp") and op.endswith("_e32"):
                    writes.add("vcc")
                elif op.startswith("v_cmp"):
                    writes.update(_sgpr_operands(parts[0]))
                elif op.startswith(("v_mad_u64_u32", "v_add_co", "v_addc_co", "v_sub_co", "v_subb_co")):
                    writes.update(_sgpr_operands(parts[1]))
                    for p in parts[2:]:
                        reads.update(x for x in _sgpr_operands(p) if CARRY.match(x))
                elif op.startswith("s_or_b64"):  # the SALU reads the compare's mask
                    reads.update(x for x in _sgpr_operands(args) if CARRY.match(x))
                for r in reads:
                    if r in last_write:
                        assert i - last_write[r] >= 3, (name, blk[last_write[r]], ins)
                        checked += 1
                for w in writes:
                    assert CARRY.match(w), w
                    last_write[w] = i
    assert checked > 200
