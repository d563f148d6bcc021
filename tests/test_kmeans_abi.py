"""The sa_kmeans_* entries and sa_dequant_lut without a GPU: the library
exports them, the header declares what sfl_amd/_lib.py binds, and the
arguments that can be refused before any launch are refused."""
import ctypes as C

import pytest
from abi_header import check_entries

from sfl_amd import _lib as L

ENTRIES = ("sa_kmeans_scratch_bytes", "sa_kmeans_hist", "sa_kmeans_step", "sa_kmeans_labels", "sa_dequant_lut")
# addresses that are never dereferenced: every call below is refused before any launch
P4, P8, ODD, ODD4 = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x1002), C.c_void_p(0x2004)


def _refused(rc, word):
    assert rc == L.SA_ERR_ARG
    assert word.encode() in L.lib().sa_last_error(), L.lib().sa_last_error()


def test_the_library_exports_the_five_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_scratch_bytes_validates_without_a_gpu():
    lib = L.lib()
    assert lib.sa_kmeans_scratch_bytes(2**32, L.SA_F32) == L.SA_ERR_ARG
    assert b"2^32" in lib.sa_last_error()
    assert lib.sa_kmeans_scratch_bytes(16, L.SA_I64) == L.SA_ERR_ARG
    for n, xt in ((2**32 - 1, L.SA_F32), (0, L.SA_F64)):
        assert lib.sa_kmeans_scratch_bytes(n, xt) == 4 * L.SA_KMEANS_BINS + L.SA_KMEANS_STATE_BYTES
    assert (4 * L.SA_KMEANS_BINS) % 8 == 0  # the state behind the histogram is 8-byte aligned


def test_every_entry_refuses_a_bad_type_or_size_before_any_launch():
    lib = L.lib()
    for n, xt, word in ((2**32, L.SA_F32, "2^32"), (16, L.SA_I64, "SA_F32 or SA_F64"), (16, 7, "SA_F32 or SA_F64")):
        _refused(lib.sa_kmeans_hist(P4, xt, n, 0.0, 1.0, P4, None), word)
        _refused(lib.sa_kmeans_step(P4, xt, n, 0.0, 1.0, 8, 1, P8, None), word)
        _refused(lib.sa_kmeans_labels(P4, xt, n, 0.0, 1.0, 8, P8, 128, P4, 1, None), word)
        _refused(lib.sa_dequant_lut(P4, 1, n, P8, 8, 128, xt, P8, P4, None), word)


def test_the_cluster_count_the_offset_and_the_code_width_are_checked():
    lib = L.lib()
    for k in (-1, 0, 1, 257, 1000):
        _refused(lib.sa_kmeans_step(P4, L.SA_F32, 16, 0.0, 1.0, k, 1, P8, None), "2..256")
        _refused(lib.sa_kmeans_labels(P4, L.SA_F32, 16, 0.0, 1.0, k, P8, 128, P4, 1, None), "2..256")
        _refused(lib.sa_dequant_lut(P4, 1, 16, P8, k, 128, L.SA_F32, P4, P4, None), "2..256")
    _refused(lib.sa_kmeans_step(P4, L.SA_F32, 16, 0.0, 1.0, 8, -1, P8, None), "steps")
    for qb in (0, 3, 4, 8, -1):
        _refused(lib.sa_kmeans_labels(P4, L.SA_F32, 16, 0.0, 1.0, 8, P8, 128, P4, qb, None), "q_bytes")
        _refused(lib.sa_dequant_lut(P4, qb, 16, P8, 8, 128, L.SA_F32, P4, P4, None), "q_bytes")
    # label - offset must stay inside the storage type: int8 holds -128 .. 127
    for k, offset, qb in ((8, 0, 1), (8, 129, 1), (200, 64, 1), (256, 127, 1), (8, 32769, 2), (8, -1, 2)):
        _refused(lib.sa_kmeans_labels(P4, L.SA_F32, 16, 0.0, 1.0, k, P8, offset, P4, qb, None), "storage type")
        _refused(lib.sa_dequant_lut(P4, qb, 16, P8, k, offset, L.SA_F32, P4, P4, None), "storage type")


def test_null_and_misaligned_pointers_are_refused():
    lib = L.lib()
    _refused(lib.sa_kmeans_hist(None, L.SA_F32, 16, 0.0, 1.0, P4, None), "required")
    _refused(lib.sa_kmeans_hist(P4, L.SA_F32, 16, 0.0, 1.0, None, None), "required")
    _refused(lib.sa_kmeans_hist(ODD, L.SA_F32, 16, 0.0, 1.0, P4, None), "aligned")
    _refused(lib.sa_kmeans_hist(P4, L.SA_F32, 16, 0.0, 1.0, ODD, None), "aligned")
    _refused(lib.sa_kmeans_step(None, L.SA_F32, 16, 0.0, 1.0, 8, 1, P8, None), "required")
    _refused(lib.sa_kmeans_step(P4, L.SA_F32, 16, 0.0, 1.0, 8, 1, None, None), "required")
    _refused(lib.sa_kmeans_step(P4, L.SA_F32, 0, 0.0, 1.0, 8, 1, None, None), "required")  # the state even for n = 0
    _refused(lib.sa_kmeans_step(ODD, L.SA_F32, 16, 0.0, 1.0, 8, 1, P8, None), "aligned")
    # a misaligned state: the sums are 64-bit words
    _refused(lib.sa_kmeans_step(P4, L.SA_F32, 16, 0.0, 1.0, 8, 1, ODD4, None), "8-byte aligned state")
    _refused(lib.sa_kmeans_step(P4, L.SA_F64, 16, 0.0, 1.0, 8, 1, ODD, None), "8-byte aligned state")
    _refused(lib.sa_kmeans_labels(P4, L.SA_F32, 16, 0.0, 1.0, 8, ODD4, 128, P4, 1, None), "8-byte aligned state")
    _refused(lib.sa_kmeans_labels(P4, L.SA_F32, 16, 0.0, 1.0, 8, None, 128, P4, 1, None), "required")
    _refused(lib.sa_kmeans_labels(None, L.SA_F32, 16, 0.0, 1.0, 8, P8, 128, P4, 1, None), "required")
    _refused(lib.sa_kmeans_labels(P4, L.SA_F32, 16, 0.0, 1.0, 8, P8, 128, None, 1, None), "required")
    _refused(lib.sa_kmeans_labels(P4, L.SA_F32, 16, 0.0, 1.0, 8, P8, 128, C.c_void_p(0x1001), 2, None), "aligned")
    _refused(lib.sa_dequant_lut(None, 1, 16, P8, 8, 128, L.SA_F32, P4, P4, None), "required")
    _refused(lib.sa_dequant_lut(P4, 1, 16, None, 8, 128, L.SA_F32, P4, P4, None), "required")
    _refused(lib.sa_dequant_lut(P4, 1, 16, P8, 8, 128, L.SA_F32, None, P4, None), "required")
    _refused(lib.sa_dequant_lut(P4, 1, 16, P8, 8, 128, L.SA_F32, P4, None, None), "required")
    _refused(lib.sa_dequant_lut(P4, 1, 16, ODD4, 8, 128, L.SA_F64, P8, P4, None), "aligned")
    _refused(lib.sa_dequant_lut(P4, 1, 16, P8, 8, 128, L.SA_F32, P4, ODD, None), "aligned")


def test_an_empty_call_launches_nothing():
    lib = L.lib()
    assert lib.sa_kmeans_labels(None, L.SA_F32, 0, 0.0, 1.0, 8, P8, 128, None, 1, None) == L.SA_OK
    assert lib.sa_dequant_lut(None, 2, 0, P8, 8, 32768, L.SA_F64, None, P4, None) == L.SA_OK
    assert lib.sa_kmeans_step(P4, L.SA_F32, 16, 0.0, 1.0, 8, 0, P8, None) == L.SA_OK  # no step


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_kmeans_scratch_bytes": "int sa_kmeans_scratch_bytes(uint64_t n, int x_type);",
        "sa_kmeans_hist": "int sa_kmeans_hist(const void* x, int x_type, uint64_t n, double mn, double s, void* hist, "
                          "void* stream);",
        "sa_kmeans_step": "int sa_kmeans_step(const void* x, int x_type, uint64_t n, double mn, double s, int k, "
                          "int steps, void* state, void* stream);",
        "sa_kmeans_labels": "int sa_kmeans_labels(const void* x, int x_type, uint64_t n, double mn, double s, int k, "
                            "const void* state, int offset, void* q_out, int q_bytes, void* stream);",
        "sa_dequant_lut": "int sa_dequant_lut(const void* q, int q_bytes, uint64_t n, const void* lut, int k, "
                          "int offset, int x_type, void* out, void* flag, void* stream);",
    }
    assert set(want) == set(ENTRIES)
    check_entries(want, (("SA_KMEANS_MAX_K", L.SA_KMEANS_MAX_K), ("SA_KMEANS_BINS", L.SA_KMEANS_BINS),
                         ("SA_KMEANS_STATE_BYTES", L.SA_KMEANS_STATE_BYTES),
                         ("SA_KMEANS_STATE_C", L.SA_KMEANS_STATE_C),
                         ("SA_KMEANS_STATE_DONE", L.SA_KMEANS_STATE_DONE)))
    check_entries({}, (("SA_KMEANS_BAD_CODE", L.SA_KMEANS_BAD_CODE),), macro_suffix="u")


def test_the_header_cites_the_references_lines_for_every_entry():
    import os
    import re

    from abi_header import ROOT

    text = open(os.path.join(ROOT, "include", "sfl_sa.h")).read()
    block = text[text.index("QuantizedKmeans: the reference's class"):text.index("#define SA_KMEANS_MAX_K")]
    for name in ENTRIES[1:]:
        at = block.index(name)
        nxt = min([block.index(o, at + 1) for o in ENTRIES[1:] if o != name and o in block[at + 1:]] + [len(block)])
        assert re.search(r"quantized_compressor\.py:231-279", block[at:nxt]), name


def test_the_wrappers_refuse_host_tensors_and_other_types():
    torch = pytest.importorskip("torch")
    from sfl_amd import kernels as K

    x, q, w = torch.ones(8), torch.zeros(8, dtype=torch.int8), torch.zeros(4096, dtype=torch.int32)
    state = torch.zeros(L.SA_KMEANS_STATE_BYTES, dtype=torch.uint8)
    with pytest.raises(ValueError, match="device-resident"):
        K.kmeans_hist(x, 0.0, 1.0, w)
    with pytest.raises(ValueError, match="device-resident"):
        K.kmeans_step(x, 0.0, 1.0, 8, 1, state)
    with pytest.raises(ValueError, match="device-resident"):
        K.kmeans_labels(x, 0.0, 1.0, 8, state, 128, q)
    with pytest.raises(ValueError, match="device-resident"):
        K.dequant_lut(q, x, 128, x, w[:2])
    with pytest.raises(TypeError):
        K.kmeans_scratch_bytes(16, torch.int64)
    assert K.kmeans_scratch_bytes(16, torch.float32) == 4 * 4096 + L.SA_KMEANS_STATE_BYTES
