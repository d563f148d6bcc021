"""The sa_quant_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, and the arguments that can be refused
before any launch are refused."""
import ctypes as C

import pytest
from abi_header import check_entries

from sfl_amd import _lib as L

ENTRIES = ("sa_quant_scratch_bytes", "sa_quant_range", "sa_quant_affine", "sa_dequant_affine", "sa_quant_fp8",
           "sa_dequant_fp8")
# addresses that are never dereferenced: every call below is refused before any launch
P4, P8, ODD = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x1002)


def test_the_library_exports_the_six_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_scratch_bytes_validates_without_a_gpu():
    lib = L.lib()
    assert lib.sa_quant_scratch_bytes(2**32, L.SA_F32) == L.SA_ERR_ARG
    assert b"2^32" in lib.sa_last_error()
    assert lib.sa_quant_scratch_bytes(16, L.SA_I64) == L.SA_ERR_ARG
    assert lib.sa_quant_scratch_bytes(2**32 - 1, L.SA_F32) > 0
    assert lib.sa_quant_scratch_bytes(0, L.SA_F64) % 8 == 0


def _refused(rc, word):
    assert rc == L.SA_ERR_ARG
    assert word.encode() in L.lib().sa_last_error(), L.lib().sa_last_error()


def test_every_entry_refuses_a_bad_type_or_size_before_any_launch():
    lib = L.lib()
    for n, xt, word in ((2**32, L.SA_F32, "2^32"), (16, L.SA_I64, "SA_F32 or SA_F64"), (16, 7, "SA_F32 or SA_F64")):
        _refused(lib.sa_quant_range(P4, xt, n, P8, P8, None), word)
        _refused(lib.sa_quant_affine(P4, xt, n, 0, 1.0, 0.0, -128, 127, P4, 1, None), word)
        _refused(lib.sa_dequant_affine(P4, 1, n, 0, 1.0, 0.0, xt, P4, None), word)
        _refused(lib.sa_quant_fp8(P4, xt, n, 1.0, 8, 6, P4, None), word)
        _refused(lib.sa_dequant_fp8(P4, n, 1.0, 8, 6, xt, P4, None), word)


def test_code_width_mode_clamp_and_format_are_checked():
    lib = L.lib()
    for qb in (0, 3, 4, 8, -1):
        _refused(lib.sa_quant_affine(P4, L.SA_F32, 16, 0, 1.0, 0.0, -128, 127, P4, qb, None), "q_bytes")
        _refused(lib.sa_dequant_affine(P4, qb, 16, 0, 1.0, 0.0, L.SA_F32, P4, None), "q_bytes")
    for mode in (-1, 2):
        _refused(lib.sa_quant_affine(P4, L.SA_F32, 16, mode, 1.0, 0.0, -128, 127, P4, 1, None), "mode")
        _refused(lib.sa_dequant_affine(P4, 2, 16, mode, 1.0, 0.0, L.SA_F64, P8, None), "mode")
    for qmin, qmax, qb in ((-129, 127, 1), (-128, 128, 1), (5, 5, 1), (7, -8, 1), (-32769, 0, 2), (0, 32768, 2)):
        _refused(lib.sa_quant_affine(P4, L.SA_F32, 16, 1, 1.0, 0.0, qmin, qmax, P4, qb, None), "storage type")
    for ml, off in ((8, 14), (4, 6), (0, 0), (16, 6), (-8, 6)):
        _refused(lib.sa_quant_fp8(P4, L.SA_F32, 16, 1.0, ml, off, P4, None), "E4M3")
        _refused(lib.sa_dequant_fp8(P4, 16, 1.0, ml, off, L.SA_F64, P8, None), "E4M3")


def test_null_and_misaligned_pointers_are_refused():
    lib = L.lib()
    # null where one is required (n > 0)
    _refused(lib.sa_quant_range(None, L.SA_F32, 16, P8, P8, None), "required")
    _refused(lib.sa_quant_range(P4, L.SA_F32, 16, None, P8, None), "required")
    _refused(lib.sa_quant_range(P4, L.SA_F32, 16, P8, None, None), "required")
    _refused(lib.sa_quant_range(None, L.SA_F32, 0, None, P8, None), "required")  # scratch and out3 even for n = 0
    _refused(lib.sa_quant_affine(None, L.SA_F32, 16, 0, 1.0, 0.0, -128, 127, P4, 1, None), "required")
    _refused(lib.sa_quant_affine(P4, L.SA_F32, 16, 0, 1.0, 0.0, -128, 127, None, 1, None), "required")
    _refused(lib.sa_dequant_affine(None, 1, 16, 0, 1.0, 0.0, L.SA_F32, P4, None), "required")
    _refused(lib.sa_dequant_affine(P4, 1, 16, 0, 1.0, 0.0, L.SA_F32, None, None), "required")
    _refused(lib.sa_quant_fp8(None, L.SA_F32, 16, 1.0, 8, 6, P4, None), "required")
    _refused(lib.sa_quant_fp8(P4, L.SA_F32, 16, 1.0, 8, 6, None, None), "required")
    _refused(lib.sa_dequant_fp8(None, 16, 1.0, 4, 14, L.SA_F32, P4, None), "required")
    _refused(lib.sa_dequant_fp8(P4, 16, 1.0, 4, 14, L.SA_F32, None, None), "required")
    # vectors that are not element-aligned
    _refused(lib.sa_quant_range(ODD, L.SA_F32, 16, P8, P8, None), "aligned")
    _refused(lib.sa_quant_range(P4, L.SA_F64, 16, ODD, P8, None), "aligned")
    _refused(lib.sa_quant_affine(ODD, L.SA_F32, 16, 0, 1.0, 0.0, -128, 127, P4, 1, None), "aligned")
    _refused(lib.sa_quant_affine(P4, L.SA_F32, 16, 0, 1.0, 0.0, -128, 127, C.c_void_p(0x1001), 2, None), "aligned")
    _refused(lib.sa_dequant_fp8(P4, 16, 1.0, 8, 6, L.SA_F64, C.c_void_p(0x1004), None), "aligned")


def test_an_empty_call_launches_nothing():
    lib = L.lib()
    assert lib.sa_quant_affine(None, L.SA_F32, 0, 0, 1.0, 0.0, -128, 127, None, 1, None) == L.SA_OK
    assert lib.sa_dequant_affine(None, 2, 0, 1, 1.0, 0.0, L.SA_F64, None, None) == L.SA_OK
    assert lib.sa_quant_fp8(None, L.SA_F32, 0, 1.0, 8, 6, None, None) == L.SA_OK
    assert lib.sa_dequant_fp8(None, 0, 1.0, 4, 14, L.SA_F64, None, None) == L.SA_OK


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_quant_scratch_bytes": "int sa_quant_scratch_bytes(uint64_t n, int x_type);",
        "sa_quant_range": "int sa_quant_range(const void* x, int x_type, uint64_t n, void* scratch, void* out3, "
                          "void* stream);",
        "sa_quant_affine": "int sa_quant_affine(const void* x, int x_type, uint64_t n, int mode, double p0, "
                           "double p1, int qmin, int qmax, void* q_out, int q_bytes, void* stream);",
        "sa_dequant_affine": "int sa_dequant_affine(const void* q, int q_bytes, uint64_t n, int mode, double p0, "
                             "double p1, int x_type, void* out, void* stream);",
        "sa_quant_fp8": "int sa_quant_fp8(const void* x, int x_type, uint64_t n, double scale, int mant_len, "
                        "int exp_offset, void* q_out, void* stream);",
        "sa_dequant_fp8": "int sa_dequant_fp8(const void* q, uint64_t n, double scale, int mant_len, "
                          "int exp_offset, int x_type, void* out, void* stream);",
    }
    assert set(want) == set(ENTRIES)
    check_entries(want, (("SA_QUANT_ZERO_POINT", L.SA_QUANT_ZERO_POINT), ("SA_QUANT_LSTM", L.SA_QUANT_LSTM)))


def test_the_wrappers_refuse_host_tensors_and_other_types():
    torch = pytest.importorskip("torch")
    from sfl_amd import kernels as K

    x, q = torch.ones(8), torch.zeros(8, dtype=torch.int8)
    with pytest.raises(ValueError, match="device-resident"):
        K.quant_range(x, q, x)
    with pytest.raises(ValueError, match="device-resident"):
        K.quant_affine(x, 0, 1.0, 0.0, -128, 127, q)
    with pytest.raises(ValueError, match="device-resident"):
        K.dequant_fp8(q, 1.0, 8, 6, x)
    with pytest.raises(TypeError):
        K.quant_scratch_bytes(16, torch.int64)
    assert K.quant_scratch_bytes(16, torch.float32) > 0
