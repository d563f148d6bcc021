"""Regenerates tests/golden/stc_reference.npz: what the reference's own
``STCSparse`` (sfl/utils/compressor/sparse_compressor.py:142-179) gives on
seeded inputs.  Run on a CPU with the reference checkout at hand:

    python tests/golden/make_stc_golden.py /path/to/reference

``sparse_compressor.py`` is loaded stand-alone: the ``sfl`` package itself
needs jax and secretflow to import, so ``sfl.utils.compressor.base`` (two
empty base classes as far as this file is concerned) is stubbed; the
``sparse`` library is only imported inside sparse_encode / sparse_decode.

Inputs: ``default_rng(seed).standard_normal(n) * 1e-2`` as float32 and
float64, n in N, rates in RATES.  Every case must have a unique threshold
magnitude (tests/stc_oracle.py ``threshold_is_unique``): the reference's
unstable argsort is then bound to mask the stable order's set.  A case that
has a tie moves on to the next seed; no case is skipped.

Per case the fixture records the seed, the support (packbits), the sign
bits of the nonzeros' positions (packbits of sparse < 0), mu_ref and
|mu_ref - mu_exact| (mu_exact from math.fsum).  Data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import stc_oracle as so  # noqa: E402

N = (1, 2, 63, 64, 65, 257, 4099, 65537)
RATES = (0.0, 0.5, 0.9, 0.99, 1.0)
DTYPES = (np.float32, np.float64)


def case_input(seed, n, dtype):
    return (np.random.default_rng(seed).standard_normal(n) * 1e-2).astype(dtype)


def load_reference(root):
    for name in ("sfl", "sfl.utils", "sfl.utils.compressor"):
        sys.modules.setdefault(name, types.ModuleType(name))
    base = types.ModuleType("sfl.utils.compressor.base")
    base.CompressedData = type("CompressedData", (), {"__init__": lambda self, d: setattr(self, "compressed_data", d)})
    base.Compressor = type("Compressor", (), {})
    sys.modules["sfl.utils.compressor.base"] = base
    path = os.path.join(root, "sfl", "utils", "compressor", "sparse_compressor.py")
    spec = importlib.util.spec_from_file_location("reference_sparse_compressor", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ["SFL_REFERENCE"])
    out = {}
    worst = 0.0
    for dt in DTYPES:
        for n in N:
            for rate in RATES:
                m = so.mask_count(rate, n)
                seed = 1000 * n + int(rate * 100)
                while not so.threshold_is_unique(case_input(seed, n, dt), m):
                    seed += 1
                u = case_input(seed, n, dt)
                assert so.threshold_is_unique(u, m)
                (sparse,) = ref.STCSparse(sparse_rate=rate)([u.copy()])
                mu_ref = float(np.max(np.abs(sparse))) if n > m else 0.0
                nz = sparse != 0
                assert np.all(np.abs(sparse[nz]) == np.abs(sparse[nz][0])) if nz.any() else True
                exact = so.mu_exact(u, m)
                key = f"{np.dtype(dt).name}_{n}_{int(rate * 100)}"
                out[key + "_seed"] = np.int64(seed)
                out[key + "_support"] = np.packbits(nz)
                out[key + "_neg"] = np.packbits(sparse < 0)
                out[key + "_mu_ref"] = np.float64(mu_ref)
                out[key + "_mu_err"] = np.float64(abs(mu_ref - exact))
                worst = max(worst, abs(mu_ref - exact) / so.ulp(exact, dt) if exact else 0.0)
    np.savez_compressed(os.path.join(HERE, "stc_reference.npz"), **out)
    print(f"{len(out) // 5} cases; worst |mu_ref - mu_exact| = {worst:.2f} ulp")


if __name__ == "__main__":
    main()
