"""The three-carry draw on the ISA the build keeps: one VALU fewer per draw in
every masking shape's tile loop, nothing else moved.

tests/test_loop_census.py keeps the bounds of the four-carry build
(1,389 VALU per headline tile).  Here the same census (tools/loop_census.py)
is held to what dropping one v_addc per draw gives: the headline
k_clients<float, float, 8, 0, 4> at 1,389 - 56 = 1,333 VALU or fewer with its
504 v_mad_u64_u32, 57 s_or_b64, at most 209 VGPRs and no scratch, and every
other pinned shape at least (draws per tile) below its earlier count.  No GPU
needed; the ISA file must exist after a build."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import loop_census  # noqa: E402


def _census(*shape):
    assert os.path.exists(loop_census.DEFAULT_ISA), (
        "the build keeps the masking kernels' ISA (sfl_amd/csrc/Makefile); run __graft_entry__.build()")
    return loop_census.census(loop_census.DEFAULT_ISA, *shape)


def test_headline_tile_loop_lost_one_valu_per_draw():
    c = _census("f", "f", 8, 0, 4)
    assert c["mad_u64"] == 504  # 56 draws of 9 v_mad_u64_u32
    assert c["valu"] <= 1333, c
    assert c["s_or_b64"] == 57, c
    assert c["vgpr"] <= 209 and c["scratch"] == 0 and c["vgpr_spill"] == 0, c
    assert c["scalar"] <= 200 and c["s_load"] <= 28 + 18 and c["s_waitcnt"] <= 24, c  # the scalar side: as it was


def test_every_shape_is_its_draws_below_the_four_carry_count():
    # (L, X, K): (VALU per tile of the four-carry build, streams) -- a tile draws each stream twice
    before = {(4, 4, 4): (1041, 22), (2, 6, 4): (611, 13), (1, 7, 6): (331, 7), (1, 32, 14): (1475, 32),
              (8, 0, 1): (771, 16), (8, 0, 0): (1565, 28)}
    for (L, X, K), (valu, streams) in before.items():
        c = _census("f", "f", L, X, K)
        draws = 2 * streams
        assert c["mad_u64"] == 9 * draws, ((L, X, K), c)
        assert c["valu"] <= valu - draws, ((L, X, K), c)
        assert c["scratch"] == 0 and c["vgpr_spill"] == 0, ((L, X, K), c)
