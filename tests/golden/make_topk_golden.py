"""Regenerates tests/golden/topk_reference.npz: what the reference's own
``TopkSparse`` (sfl/utils/compressor/sparse_compressor.py:23-139) and
``MixedCompressor`` (mixed_compressor.py:23-111) give on seeded inputs, under
numpy 2 and scipy.  Run on a CPU with the reference checkout at hand:

    python tests/golden/make_topk_golden.py /path/to/reference

The three files are loaded stand-alone: the ``sfl`` package itself needs jax
and secretflow to import, so ``sfl.utils.compressor`` and its ``base`` are
stubbed (``CompressedData`` holds one field; ``Compressor`` maps
``_compress_one`` / ``_decompress_one`` over one object or a list, which is
all the three files use of it).

Inputs (tests/topk_cases.py): ``default_rng(seed).standard_normal(shape) * s``
as float32 and float64, every shape of SHAPES at every rate of RATES.  A case
whose k-th and (k+1)-th largest keys are equal (the reference's argpartition
would break that tie arbitrarily) moves on to the next seed; no case is
skipped.  Per case the fixture records the seed, k, the sha256 of the
reference's decompressed bytes, and the same for the ``sparse_mask`` round
trip (compress again with the first result's mask).

MixedCompressor: TopkSparse(0.9) with QuantizedZeroPoint and QuantizedLSTM at
8 bits.  Recorded: the codes, **in ascending flat-index order** (the reference
holds them in argpartition's order, on which no code depends), and the sha256
of the decompressed array.  An LSTM case whose reference result would leave
the storage range (the reference's cast would wrap where this project
saturates) moves on to the next seed, as in make_quant_golden.py.  Data only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import topk_cases as tc  # noqa: E402


def load_reference(root):
    class CompressedData:
        def __init__(self, compressed_data):
            self.compressed_data = compressed_data

    class Compressor:
        def compress(self, data, **kwargs):
            if isinstance(data, (list, tuple)):
                return [self._compress_one(d, **kwargs) for d in data]
            return self._compress_one(data, **kwargs)

        def decompress(self, data):
            if isinstance(data, list):
                return [self._decompress_one(d) for d in data]
            return self._decompress_one(data)

        def iscompressed(self, data):
            return isinstance(data, CompressedData)

    for name in ("sfl", "sfl.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    pkg = types.ModuleType("sfl.utils.compressor")
    pkg.__path__ = []  # a package: mixed_compressor.py imports its siblings relatively
    pkg.CompressedData = CompressedData
    base = types.ModuleType("sfl.utils.compressor.base")
    base.CompressedData, base.Compressor = CompressedData, Compressor
    sys.modules["sfl.utils.compressor"] = pkg
    sys.modules["sfl.utils.compressor.base"] = base
    mods = {}
    for short in ("quantized_compressor", "sparse_compressor", "mixed_compressor"):
        full = "sfl.utils.compressor." + short
        path = os.path.join(root, "sfl", "utils", "compressor", short + ".py")
        spec = importlib.util.spec_from_file_location(full, path)
        mods[short] = sys.modules[full] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[short])
    return mods


def leaves_storage(scheme, quantized, values):
    """Would the reference's LSTM cast wrap on these values?"""
    if not scheme.startswith("lstm"):
        return False
    info = np.iinfo(np.int8)
    v = np.round(quantized.q * values) - quantized.rqm
    return bool(v.min() < info.min or v.max() > info.max)


def main():
    assert int(np.__version__.split(".")[0]) >= 2, "the definition is numpy 2's (NEP 50)"
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ["SFL_REFERENCE"])
    sparse_mod, quant_mod, mixed_mod = ref["sparse_compressor"], ref["quantized_compressor"], ref["mixed_compressor"]
    out, table, moved = {}, [], 0
    zero = np.zeros(32, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for k, si, ri, dt in tc.all_cases():
            shape, rate = tc.SHAPES[si], tc.RATES[ri]
            kept = tc.keep_count(rate, tc.size(shape))
            seed = tc.first_seed(si, ri, dt)
            while tc.tie_at_threshold(tc.case_input(seed, shape, tc.scale_of(ri), dt), kept):
                seed, moved = seed + 1, moved + 1
            x = tc.case_input(seed, shape, tc.scale_of(ri), dt)
            comp = sparse_mod.TopkSparse(rate)
            c = comp.compress(x.copy())
            assert len(c.compressed_data) == kept, (k, len(c.compressed_data), kept)
            dec = comp.decompress(c)
            assert dec.dtype == x.dtype and dec.shape == x.shape, (k, dec.dtype, dec.shape)
            dec2 = comp.decompress(comp.compress(x.copy(), sparse_mask=c.get_sparse_mask()))
            assert dec2.dtype == x.dtype and dec2.shape == x.shape, (k, dec2.dtype, dec2.shape)
            table.append((k, seed, kept, tc.digest(dec), tc.digest(dec2)))
        for k, scheme, si, dt in tc.mixed_cases():
            shape = tc.SHAPES[si]
            cls, kw = tc.MIXED[scheme]
            kept = tc.keep_count(tc.MIXED_RATE, tc.size(shape))
            seed = tc.first_seed(si, 50 + list(tc.MIXED).index(scheme), dt)
            while True:
                x = tc.case_input(seed, shape, tc.SCALES[1], dt)
                comp = mixed_mod.MixedCompressor(sparse_mod.TopkSparse(tc.MIXED_RATE), getattr(quant_mod, cls)(**kw))
                c = comp.compress(x.copy())
                sparse_data, quantized = c.compressed_participants
                values = x.reshape(sparse_data.shape)[sparse_data.row, sparse_data.col]
                if not tc.tie_at_threshold(x, kept) and not leaves_storage(scheme, quantized, values):
                    break
                seed, moved = seed + 1, moved + 1
            order = np.argsort(sparse_data.row.astype(np.int64) * sparse_data.shape[1] + sparse_data.col)
            out[k + "_codes"] = np.asarray(c.compressed_data)[order]
            dec = comp.decompress(c)
            assert dec.dtype == x.dtype and dec.shape == x.shape, (k, dec.dtype, dec.shape)
            table.append((k, seed, kept, tc.digest(dec), zero))
    out["keys"] = np.array([t[0] for t in table])
    out["seed"] = np.array([t[1] for t in table], dtype=np.int64)
    out["k"] = np.array([t[2] for t in table], dtype=np.int64)
    out["dec"] = np.stack([t[3] for t in table])
    out["dec_mask"] = np.stack([t[4] for t in table])
    np.savez_compressed(tc.GOLDEN, **out)
    print(f"{len(table)} cases, {moved} seeds moved on; {os.path.getsize(tc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
