"""The scalar side of the masking kernel's tile loop, pinned on the ISA the
build keeps (sfl_amd/csrc/Makefile: -save-temps of sa_clients_f32.hip).

At two waves per SIMD every scalar instruction, scalar load and s_waitcnt at
the head of a wave is an issue turn without VALU work, so the
8-client sum-only launch k_clients<float, float, 8, 0, 4> keeps, per tile of
its fast path (tools/loop_census.py): at most 200 scalar-side instructions
(314 before the draw groups' constants came in two loads per group), at most
1,389 VALU, at most 224 VGPRs and no scratch.  No GPU needed; the ISA file
must exist after a build."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import loop_census  # noqa: E402


def _census(*shape):
    assert os.path.exists(loop_census.DEFAULT_ISA), (
        "the build keeps the masking kernels' ISA (sfl_amd/csrc/Makefile); run __graft_entry__.build()")
    return loop_census.census(loop_census.DEFAULT_ISA, *shape)


def test_headline_tile_loop_budget():
    c = _census("f", "f", 8, 0, 4)
    assert c["mad_u64"] == 504  # 56 draws of 9 v_mad_u64_u32: the whole mask expansion is in the walk
    assert c["scalar"] <= 200, c
    assert c["valu"] <= 1389, c
    assert c["vgpr"] <= 224 and c["scratch"] == 0 and c["vgpr_spill"] == 0, c
    # one zero-test OR per draw (+1 joining the two element slots), two loads per draw group
    assert c["s_or_b64"] == 57 and c["s_load"] <= 28 + 18 and c["s_waitcnt"] <= 24, c


def test_shapes_sharing_the_layout_keep_their_valu_count():
    """The per-rank shapes and the masks-only launches run the same header:
    their tile loops' VALU counts are the draws' (no spill code came in) and
    their scalar side went down with the headline's."""
    want = {(4, 4, 4): (1041, 245), (2, 6, 4): (611, 165), (1, 7, 6): (331, 104), (1, 32, 14): (1475, 274),
            (8, 0, 1): (771, 177), (8, 0, 0): (1565, 457)}
    for (L, X, K), (valu, scalar_before) in want.items():
        c = _census("f", "f", L, X, K)
        assert c["valu"] <= valu and c["scalar"] < scalar_before and c["scratch"] == 0, ((L, X, K), c)


def test_census_tool_prints_the_table():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_census.py")], capture_output=True,
                         text=True, check=True).stdout
    assert "| scalar side, total |" in out and "504 v_mad_u64_u32" in out
