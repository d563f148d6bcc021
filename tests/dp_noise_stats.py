"""Statistics of a Gaussian noise stream and the Box-Muller extremes (test
helper, shared by tests/test_dp_oracle.py and tests/test_gpu_dp_noise.py).

Every bound is a formula: five standard errors of the exact N(0,1) sampling
distribution of the statistic at the sample's size, or the Dvoretzky-Kiefer-
Wolfowitz bound at 1e-9 for the empirical CDF.  None is a measured number.
Only ``math.erf`` is needed (no scipy).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import dp as D

KEY = 0x5EED0D9A11CE0001
N = 1 << 22
RTOL, ATOL = 2e-5, 2e-6  # |z - z64| <= RTOL |z64| + ATOL (tests/test_gpu_dp.py's tolerance)

LAGS = (1, 2, 3, 4, 5, 8, 1024)
TAILS = (2.0, 3.0, 4.0)
CDF_GRID = np.linspace(-6.0, 6.0, 2401)
CDF_PHI = np.array([0.5 * (1.0 + math.erf(t / math.sqrt(2.0))) for t in CDF_GRID])


def _corr(a: np.ndarray, b: np.ndarray) -> float:
    a = a - a.mean()
    b = b - b.mean()
    return float(np.dot(a, b) / math.sqrt(float(np.dot(a, a)) * float(np.dot(b, b))))


def noise_statistics(z, other_key=None, next_window=None) -> dict:
    """{name: (value, bound)} of the sample ``z`` (taken as float64):
    moments, the empirical CDF against Phi on ``CDF_GRID``, the tail counts
    (in binomial standard deviations), autocorrelations at ``LAGS`` and, when
    given, the correlation with the stream of another key at the same
    counters and with the same key's next window."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    n = z.size
    se = 5.0 / math.sqrt(n)
    m = float(z.mean())
    d = z - m
    d2 = d * d
    var = float(d2.mean())
    out = {
        "mean": (m, se),
        "variance - 1": (var - 1.0, 5.0 * math.sqrt(2.0 / n)),
        "skewness": (float((d2 * d).mean()) / var**1.5, 5.0 * math.sqrt(6.0 / n)),
        "excess kurtosis": (float((d2 * d2).mean()) / var**2 - 3.0, 5.0 * math.sqrt(24.0 / n)),
    }
    ecdf = np.searchsorted(np.sort(z), CDF_GRID, side="right") / n
    out["max |ECDF - Phi|"] = (float(np.abs(ecdf - CDF_PHI).max()), math.sqrt(math.log(2e9) / (2.0 * n)))
    az = np.abs(z)
    for t in TAILS:
        p = 1.0 - math.erf(t / math.sqrt(2.0))
        out[f"count |z| > {t:g} (sd)"] = ((int((az > t).sum()) - n * p) / math.sqrt(n * p * (1.0 - p)), 5.0)
    for k in LAGS:
        out[f"autocorrelation lag {k}"] = (float(np.dot(d[:-k], d[k:])) / (n * var), se)
    if other_key is not None:
        out["correlation with key + 1"] = (_corr(z, np.asarray(other_key, dtype=np.float64).reshape(-1)), se)
    if next_window is not None:
        out["correlation with the next window"] = (_corr(z, np.asarray(next_window, dtype=np.float64).reshape(-1)),
                                                   se)
    return out


def check_noise_statistics(stats: dict, who: str) -> None:
    """Print every figure, then assert each within its bound."""
    for name, (v, b) in stats.items():
        print(f"{who}: {name} = {v:+.4g} (bound {b:.4g})")
    bad = {name: vb for name, vb in stats.items() if not abs(vb[0]) <= vb[1]}
    assert not bad, f"{who}: outside the bound: {bad}"


def worst_element(z, z64, words_of) -> str:
    """The element of ``z`` furthest outside RTOL |z64| + ATOL, with its two
    Philox words (``words_of(e)`` -> (w_u1, w_u2)); '' when all are inside."""
    z = np.asarray(z, dtype=np.float64)
    err = np.abs(z - z64)
    tol = RTOL * np.abs(z64) + ATOL
    with np.errstate(invalid="ignore"):
        over = np.where(np.isfinite(z), err / tol, np.inf)
    e = int(np.argmax(over))
    if over[e] <= 1.0:
        return ""
    w0, w1 = words_of(e)
    return (f"{int((over > 1.0).sum())} of {z.size} elements outside {RTOL:g} |z64| + {ATOL:g}; worst element {e}: "
            f"got {z[e]!r}, float64 reference {z64[e]!r}, error {err[e]:.3e} = {over[e]:.2f} x the tolerance, "
            f"Philox words u1 <- {w0:#010x}, u2 <- {w1:#010x}")


def stream_words_of(key: int, counter0: int):
    """``words_of`` for ``worst_element`` on the stream (key, counter0)."""
    def f(e):
        g = counter0 + e
        w = D.philox_words(key, 4 * (g // 4), 4)[0]
        j = (g >> 1) & 1
        return int(w[2 * j]), int(w[2 * j + 1])

    return f


# The Box-Muller inputs where an approximate log / sin / cos unit is at its
# worst, each of probability 2^-24 per word: (name, block, pair j, which word
# of the pair (0: the u1 word, 1: the u2 word), its 24-bit value w >> 8), found
# by a scan of the first 2^25 blocks of KEY.  test_dp_oracle.py recomputes
# the words, so these cannot rot.  Joint extremes (u1 at its minimum AND u2
# at a quarter turn) have probability 2^-48 per pair and are out of reach of
# any scan.
EXTREMES = (
    ("u1 minimum (2^-24, radius 5.768)", 1248306, 1, 0, 0x000000),
    ("u1 minimum (2^-24, radius 5.768)", 9397138, 1, 0, 0x000000),
    ("u1 minimum (2^-24, radius 5.768)", 10493971, 1, 0, 0x000000),
    ("u1 = 1 (radius sqrt(-0.0))", 1852138, 0, 0, 0xFFFFFF),
    ("u1 = 1 (radius sqrt(-0.0))", 5633351, 1, 0, 0xFFFFFF),
    ("u1 = 1 (radius sqrt(-0.0))", 9377376, 0, 0, 0xFFFFFF),
    ("u2 = 0", 3764981, 0, 1, 0x000000),
    ("u2 = 0", 24356043, 1, 1, 0x000000),
    ("u2 = 1/4 - 2^-24", 1471904, 0, 1, 0x3FFFFF),
    ("u2 = 1/4 - 2^-24", 5008479, 1, 1, 0x3FFFFF),
    ("u2 = 1/4", 1663657, 0, 1, 0x400000),
    ("u2 = 1/4", 998155, 1, 1, 0x400000),
    ("u2 = 1/4", 9110760, 0, 1, 0x400000),
    ("u2 = 1/4 + 2^-24", 11751453, 1, 1, 0x400001),
    ("u2 = 1/2", 5499226, 0, 1, 0x800000),
    ("u2 = 1/2", 8546072, 0, 1, 0x800000),
    ("u2 = 1/2", 21380075, 1, 1, 0x800000),
    ("u2 = 3/4", 30626795, 1, 1, 0xC00000),
    ("u2 maximum (1 - 2^-24)", 22636863, 1, 1, 0xFFFFFF),
)

# float64 reference (z0, z1) of the first hit of each target's pair, as the
# scan recorded it (tests/test_dp_oracle.py holds gauss64 to these)
EXTREME_PAIRS = {
    1248306: (3.79692834, -4.34216534),
    1852138: (0.0, -0.0),
    3764981: (1.24156996, 0.0),
    1471904: (3.3457e-7, 0.89335996),
    1663657: (0.0, 0.544463194),
    11751453: (-3.8137e-7, 1.01833742),
    5499226: (-1.56154253, 0.0),
    30626795: (0.0, -0.450015953),
    22636863: (1.28211862, -4.8016e-7),
}
