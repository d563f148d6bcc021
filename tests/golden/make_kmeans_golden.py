"""Regenerates tests/golden/kmeans_reference.npz: what the reference's own
``QuantizedKmeans`` (sfl/utils/compressor/quantized_compressor.py:231-279,
scikit-learn's ``KMeans(K, n_init=1, max_iter=50)``) gives on seeded inputs.
Run on a CPU with scikit-learn and the reference checkout at hand:

    python tests/golden/make_kmeans_golden.py /path/to/reference

The module is loaded stand-alone as in make_quant_golden.py (the ``sfl``
package needs jax and secretflow to import).  The reference's start is random,
so every case runs five times, ``km.set_params(random_state=s)`` for ``s`` in
0..4, and the fixture records each run's sum of squared errors
(``sse``, cases x 5, rows in ``keys``' order): the yardstick of
test_kmeans_host.py's quality cap.  For the normal float32 K = 8 case, run 0,
it also records the reference's int8 codes, ``q`` and the decompressed array,
for the decode parity test.

Inputs (tests/kmeans_cases.py ``data``) are regenerated from their seeds; only
results are stored.  Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import kmeans_cases as kc  # noqa: E402
from make_quant_golden import load_reference  # noqa: E402


def main():
    import sklearn

    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ["SFL_REFERENCE"])
    out, keys, table = {}, [], []
    for kind, dt, K in kc.all_cases():
        x = kc.data(kind, dt)
        row = []
        for s in kc.SEEDS:
            comp = ref.QuantizedKmeans(quant_bits=8, n_clusters=K)
            comp.km.set_params(random_state=s)
            c = comp._compress_one(x.copy())
            dec = comp._decompress_one(c)
            assert dec.shape == x.shape and dec.dtype == x.dtype, (kind, dt, K, dec.dtype)
            row.append(kc.sse(x, dec))
            if (kind, dt, K) == kc.CODES_CASE and s == 0:
                assert c.compressed_data.dtype == np.int8 and c.q.shape == (K, 1)
                out["codes"], out["q"], out["dec"] = c.compressed_data, c.q, dec
        keys.append(kc.key(kind, dt, K))
        table.append(row)
        print(keys[-1], " ".join(f"{v:.6g}" for v in row), flush=True)
    out["keys"] = np.array(keys)
    out["sse"] = np.array(table, dtype=np.float64)
    out["sklearn"] = np.array(sklearn.__version__)
    np.savez_compressed(kc.GOLDEN, **out)
    print(f"{len(keys)} cases; {os.path.getsize(kc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
