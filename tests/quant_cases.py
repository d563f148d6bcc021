"""The cases of tests/golden/quant_reference.npz: shared by its generator
(tests/golden/make_quant_golden.py) and the tests that read it."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant_reference.npz")

N = (2, 3, 63, 64, 65, 257, 4099)
SCALES = (1e-2, 5)
DTYPES = (np.float32, np.float64)
# scheme -> (class name, constructor arguments)
SCHEMES = {
    "zp8": ("QuantizedZeroPoint", dict(quant_bits=8)),
    "zp16": ("QuantizedZeroPoint", dict(quant_bits=16)),
    "zp4": ("QuantizedZeroPoint", dict(quant_bits=4)),
    "lstm8": ("QuantizedLSTM", dict(quant_bits=8)),
    "lstm16": ("QuantizedLSTM", dict(quant_bits=16)),
    "e4m3": ("QuantizedFP", dict(quant_bits=8, format="E4M3")),
    "e5m2": ("QuantizedFP", dict(quant_bits=8, format="E5M2")),
}
FP8 = {"e4m3": (448, 8, 6), "e5m2": (57344, 4, 14)}  # max_value, mant_len, exp_offset


def case_input(seed, n, s, dtype):
    return (np.random.default_rng(seed).standard_normal(n) * s).astype(dtype)


def first_seed(n, si, dtype):
    return 100000 * n + 1000 * si + 8 * np.dtype(dtype).itemsize


def zero_point_ties(dtype):
    """scale = 2^-8 and z = 0 exactly; every other element is a rounding tie.
    Round-half-away would get 128 of the codes wrong."""
    k = np.arange(-128, 127)
    return np.concatenate([[-128 / 256, 127 / 256], (k + 0.5) / 256]).astype(dtype)


def fp8_ties(scheme, dtype):
    """scale = 1 exactly; every mantissa tie of every exponent from three
    below the least coded one to the top, the qm = mant_len carry included."""
    max_value, ml, off = FP8[scheme]
    _, top = np.frexp(np.float64(max_value))
    out = [float(max_value)]
    for e in range(-off - 3, int(top) + 1):
        for k in range(ml):
            v = float(np.ldexp(((k + 0.5) / ml + 1) / 2, e))
            if v <= max_value:
                out += [v, -v]
    return np.asarray(out, dtype=dtype)


def tie_input(scheme, dtype):
    return zero_point_ties(dtype) if scheme == "zp8" else fp8_ties(scheme, dtype)


def lstm_saturating(bits, dtype, n=3):
    """q = 1 and rqm = 2^(bits-1) exactly; the largest element's code is
    +2^(bits-1) before the clamp, one past the storage range.  n > 3 repeats
    the three values."""
    return np.resize(np.array([0.5, 3.0, (1 << bits) - 0.5], dtype=dtype), n)


TIE_SCHEMES = ("zp8", "e4m3", "e5m2")


def key(scheme, dtype, n, si):
    return f"{scheme}_{np.dtype(dtype).name}_{n}_{si}"


def tie_key(scheme, dtype):
    return f"tie_{scheme}_{np.dtype(dtype).name}"


def digest(a) -> np.ndarray:
    """sha256 of an array's bytes (C order), as 32 uint8."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def params_of(scheme, c):
    """A compressed object's scalars as two float64 (exact for the data's type) / integers."""
    if scheme.startswith("zp"):
        return np.float64(c.scale), np.int64(c.nudged_zero_point)
    if scheme.startswith("lstm"):
        return np.float64(c.q), np.int64(c.rqm)
    return np.float64(c.scale), np.int64(0)


def all_cases():
    """(key, scheme, dtype, n, scale index) of every random case."""
    for scheme in SCHEMES:
        for dt in DTYPES:
            for n in N:
                for si in range(len(SCALES)):
                    yield key(scheme, dt, n, si), scheme, dt, n, si


class Golden:
    """The fixture: per case the codes (``<key>_codes``); the seeds, scalars
    and digests of all cases in tables indexed by ``keys``."""

    def __init__(self, path=GOLDEN):
        self.z = np.load(path)
        self.row = {k: i for i, k in enumerate(self.z["keys"].tolist())}

    def codes(self, k):
        return self.z[k + "_codes"]

    def seed(self, k):
        return int(self.z["seed"][self.row[k]])

    def params(self, k):
        return self.z["p0"][self.row[k]], self.z["p1"][self.row[k]]

    def dec(self, k):
        return self.z["dec"][self.row[k]]
