"""Regenerates tests/golden/quant_reference.npz: what the reference's own
``QuantizedZeroPoint``, ``QuantizedLSTM`` and ``QuantizedFP``
(sfl/utils/compressor/quantized_compressor.py:65-228) give on seeded inputs,
under numpy 2 (NEP 50).  Run on a CPU with the reference checkout at hand:

    python tests/golden/make_quant_golden.py /path/to/reference

``quantized_compressor.py`` is loaded stand-alone: the ``sfl`` package itself
needs jax and secretflow to import, so ``sfl.utils.compressor`` and its
``base`` (two empty base classes as far as this file is concerned) are
stubbed, and ``_compress_one`` / ``_decompress_one`` are called directly.

Inputs (tests/quant_cases.py): ``default_rng(seed).standard_normal(n) * s``
as float32 and float64, n in N, s in SCALES, every scheme of SCHEMES; and the
tie sets of zero-point and of the two fp8 formats.  An LSTM case whose
reference result would leave the storage range (the reference's cast would
wrap where this project saturates) moves on to the next seed; no case is
skipped.

Per case the fixture records the codes (``<key>_codes``) and, in tables
indexed by ``keys``, the seed, the scalars and the sha256 of the decompressed
array's bytes (tests/quant_cases.py ``Golden`` reads them).  Data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import quant_cases as qc  # noqa: E402


def load_reference(root):
    class CompressedData:
        def __init__(self, compressed_data):
            self.compressed_data = compressed_data

    for name in ("sfl", "sfl.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    pkg = types.ModuleType("sfl.utils.compressor")
    pkg.CompressedData = CompressedData
    base = types.ModuleType("sfl.utils.compressor.base")
    base.CompressedData = CompressedData
    base.Compressor = type("Compressor", (), {"__init__": lambda self: None})
    sys.modules["sfl.utils.compressor"] = pkg
    sys.modules["sfl.utils.compressor.base"] = base
    path = os.path.join(root, "sfl", "utils", "compressor", "quantized_compressor.py")
    spec = importlib.util.spec_from_file_location("reference_quantized_compressor", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def leaves_storage(scheme, comp, c, x):
    """Would the reference's LSTM cast wrap on this input?"""
    if not scheme.startswith("lstm"):
        return False
    info = np.iinfo(comp.np_type)
    v = np.round(c.q * x) - c.rqm
    return bool(v.min() < info.min or v.max() > info.max)


def record(out, table, k, scheme, comp, x, seed):
    c = comp._compress_one(x.copy())
    dec = comp._decompress_one(c)
    assert dec.dtype == x.dtype and dec.shape == x.shape, (k, dec.dtype)
    p0, p1 = qc.params_of(scheme, c)
    assert x.dtype.type(p0) == p0, k  # the scalar has the data's type
    out[k + "_codes"] = c.compressed_data
    table.append((k, seed, p0, p1, qc.digest(dec)))


def main():
    assert int(np.__version__.split(".")[0]) >= 2, "the definition is numpy 2's (NEP 50)"
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ["SFL_REFERENCE"])
    out, table, moved = {}, [], 0
    with np.errstate(all="ignore"):
        for k, scheme, dt, n, si in qc.all_cases():
            cls, kw = qc.SCHEMES[scheme]
            comp = getattr(ref, cls)(**kw)
            seed = qc.first_seed(n, si, dt)
            while True:
                x = qc.case_input(seed, n, qc.SCALES[si], dt)
                if not leaves_storage(scheme, comp, comp._compress_one(x.copy()), x):
                    break
                seed, moved = seed + 1, moved + 1
            record(out, table, k, scheme, comp, x, seed)
        for scheme in qc.TIE_SCHEMES:
            cls, kw = qc.SCHEMES[scheme]
            for dt in qc.DTYPES:
                record(out, table, qc.tie_key(scheme, dt), scheme, getattr(ref, cls)(**kw), qc.tie_input(scheme, dt), -1)
    out["keys"] = np.array([t[0] for t in table])
    out["seed"] = np.array([t[1] for t in table], dtype=np.int64)
    out["p0"] = np.array([t[2] for t in table], dtype=np.float64)
    out["p1"] = np.array([t[3] for t in table], dtype=np.int64)
    out["dec"] = np.stack([t[4] for t in table])
    np.savez_compressed(qc.GOLDEN, **out)
    print(f"{len(table)} cases, {moved} LSTM seeds moved on; {os.path.getsize(qc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
