"""The cases of tests/golden/topk_reference.npz: shared by its generator
(tests/golden/make_topk_golden.py) and the tests that read it."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_reference.npz")

SHAPES = ((10, 10), (10, 10, 10, 10), (7, 33), (3, 5, 7), (1, 300), (300, 1), (1000, 37))
RATES = (0.9, 0.5, 0.99, 0.0, 0.37)
SCALES = (1e-2, 5)
DTYPES = (np.float32, np.float64)
# MixedCompressor: TopkSparse(MIXED_RATE) + the quantizer
MIXED_RATE = 0.9
MIXED = {"zp8": ("QuantizedZeroPoint", dict(quant_bits=8)), "lstm8": ("QuantizedLSTM", dict(quant_bits=8))}


def size(shape):
    return int(np.prod(shape, dtype=np.int64))


def keep_count(rate, n):
    return round((1 - rate) * n)


def scale_of(ri):
    return SCALES[ri % len(SCALES)]


def case_input(seed, shape, s, dtype):
    return (np.random.default_rng(seed).standard_normal(shape) * s).astype(dtype)


def first_seed(si, ri, dtype):
    return 7000000 + 10000 * si + 100 * ri + 8 * np.dtype(dtype).itemsize


def abs_key(flat):
    """The bit pattern of |x| as an unsigned integer."""
    if flat.dtype == np.float32:
        return flat.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return flat.view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)


def tie_at_threshold(x, k):
    """Are the k-th and the (k+1)-th largest keys equal?"""
    key = np.sort(abs_key(np.ascontiguousarray(x).reshape(-1)))
    n = key.size
    return bool(0 < k < n and key[n - k] == key[n - k - 1])


def key(shape, ri, dtype):
    return f"topk_{'x'.join(map(str, shape))}_{ri}_{np.dtype(dtype).name}"


def mixed_key(scheme, shape, dtype):
    return f"mixed_{scheme}_{'x'.join(map(str, shape))}_{np.dtype(dtype).name}"


def digest(a) -> np.ndarray:
    """sha256 of an array's bytes (C order), as 32 uint8."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def all_cases():
    """(key, shape index, rate index, dtype) of every TopkSparse case."""
    for si, shape in enumerate(SHAPES):
        for ri in range(len(RATES)):
            for dt in DTYPES:
                yield key(shape, ri, dt), si, ri, dt


def mixed_cases():
    """(key, scheme, shape index, dtype) of every MixedCompressor case."""
    for scheme in MIXED:
        for si, shape in enumerate(SHAPES):
            for dt in DTYPES:
                yield mixed_key(scheme, shape, dt), scheme, si, dt


class Golden:
    """The fixture: the seeds, kept counts and digests of all cases in tables
    indexed by ``keys``; per MixedCompressor case the codes in index order
    (``<key>_codes``)."""

    def __init__(self, path=GOLDEN):
        self.z = np.load(path)
        self.row = {k: i for i, k in enumerate(self.z["keys"].tolist())}

    def seed(self, k):
        return int(self.z["seed"][self.row[k]])

    def k(self, k):
        return int(self.z["k"][self.row[k]])

    def dec(self, k):
        return self.z["dec"][self.row[k]]

    def dec_mask(self, k):
        return self.z["dec_mask"][self.row[k]]

    def codes(self, k):
        return self.z[k + "_codes"]
