"""The masking launch's grid choice (sfl_amd/csrc/pcg128.h: carry_free,
qualifying_grid), from a small host program against Python integers.

The three-carry draw is exact only for a multiplier with a0 + a1 + 1 <= 2^32
(its two low limbs), and the tile jump's multiplier is A^(grid*512 - 1), so
launch_clients takes its grid from qualifying_grid.  tests/c_abi/
grid_choice.cpp prints the predicate for the grids 1..2048 and the choice
for 1..2048 tiles at five caps (256, 496, 511 and 512: the headline's
occupancy with and without a masking reserve; 1792: the lean shape's); both
are recomputed here with pow(A, g*512 - 1, 2**128).  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "grid_choice.cpp")
A = 0x2360ED051FC65DA44385DF649FCCF645
M32 = (1 << 32) - 1
CAPS = (256, 496, 511, 512, 1792)


def _qualifies(g):
    m = pow(A, g * 512 - 1, 1 << 128)
    return (m & M32) + ((m >> 32) & M32) + 1 <= 1 << 32


QUAL = {g: _qualifies(g) for g in range(1, 2049)}


def _choice(tiles, cap):
    want = min(tiles, cap)
    for g in range(want, cap + 1):
        if QUAL[g]:
            return g
    for g in range(want - 1, 0, -1):
        if QUAL[g]:
            return g
    return 0


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("grid_choice") / "grid_choice")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return [ln.split() for ln in out.splitlines()]


def test_carry_free_equals_python_pow(program_output):
    got = {int(r[1]): bool(int(r[2])) for r in program_output if r[0] == "cf"}
    assert got == QUAL


def test_qualifying_grid_equals_python_search(program_output):
    got = {(int(r[1]), int(r[2])): int(r[3]) for r in program_output if r[0] == "qg"}
    assert len(got) == len(CAPS) * 2048
    for cap in CAPS:
        for t in range(1, 2049):
            g = got[(cap, t)]
            assert g == _choice(t, cap), (cap, t)
            assert 1 <= g <= cap and QUAL[g], (cap, t, g)
    # the choices the header static_asserts
    for (t, cap), g in {(1, 512): 2, (6, 512): 8, (7, 512): 8, (9, 512): 11, (16, 512): 20, (64, 512): 64,
                        (512, 512): 512}.items():
        assert got[(cap, t)] == g
    big = 10 ** 6
    assert [_choice(big, c) for c in (512, 511, 496, 256)] == [512, 508, 495, 255]
    assert [got[(c, 2048)] for c in (512, 511, 496, 256)] == [512, 508, 495, 255]  # tiles >= cap: the same branch


def test_density_of_qualifying_grids():
    """1,048 of the grids 1..2048 qualify and no run of non-qualifying grids
    is longer than 8, so the chosen grid is within 8 blocks of the wanted one."""
    assert sum(QUAL.values()) == 1048
    run = longest = 0
    for g in range(1, 2049):
        run = 0 if QUAL[g] else run + 1
        longest = max(longest, run)
    assert longest == 8
    assert QUAL[512] and not QUAL[511]
    m = pow(A, 511 * 512 - 1, 1 << 128)
    assert (m & M32, (m >> 32) & M32) == (0x1C49948D, 0xF86F8A20)
    m = pow(A, 512 * 512 - 1, 1 << 128)
    assert (m & M32, (m >> 32) & M32) == (0x5B9EAC8D, 0x2C356D7A)
    assert (A & M32) + ((A >> 32) & M32) + 1 == 0xE352D5AA  # PCG64's own multiplier: the plain step
