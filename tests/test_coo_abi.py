"""The sa_coo_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, and the arguments that can be refused
before any launch are refused."""
import pytest
from abi_header import check_entries

from sfl_amd import _lib as L

ENTRIES = ("sa_coo_scratch_bytes", "sa_coo_count", "sa_coo_fill", "sa_coo_decode", "sa_coo_axpy", "sa_coo_finish")


def test_the_library_exports_the_six_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_scratch_bytes_validates_without_a_gpu():
    lib = L.lib()
    assert lib.sa_coo_scratch_bytes(2**31, L.SA_F32) == L.SA_ERR_ARG
    assert b"2^31" in lib.sa_last_error()
    assert lib.sa_coo_scratch_bytes(2**32, L.SA_F32) == L.SA_ERR_ARG
    assert lib.sa_coo_scratch_bytes(16, L.SA_I64) == L.SA_ERR_ARG
    assert lib.sa_coo_scratch_bytes(16, L.SA_F64) > 0
    assert lib.sa_coo_scratch_bytes(2**31 - 1, L.SA_F32) > 0


def test_every_entry_refuses_a_bad_type_or_size_before_any_launch():
    lib = L.lib()
    for n, xt in ((2**31, L.SA_F32), (16, L.SA_I64)):
        assert lib.sa_coo_count(None, xt, n, None, None, None) == L.SA_ERR_ARG
        assert lib.sa_coo_fill(None, xt, n, None, None, None, 0, None, None) == L.SA_ERR_ARG
        assert lib.sa_coo_decode(None, None, xt, 0, n, None, None, None) == L.SA_ERR_ARG
        assert lib.sa_coo_axpy(None, None, xt, 0, 1.0, None, L.SA_F64, n, None, None) == L.SA_ERR_ARG
        assert lib.sa_coo_finish(None, xt, n, 2.0, None) == L.SA_ERR_ARG
    # float64 data cannot be summed in float32; an integer accumulator does not exist
    assert lib.sa_coo_axpy(None, None, L.SA_F64, 0, 1.0, None, L.SA_F32, 16, None, None) == L.SA_ERR_ARG
    assert lib.sa_coo_axpy(None, None, L.SA_F32, 0, 1.0, None, L.SA_I64, 16, None, None) == L.SA_ERR_ARG
    # null pointers where one is required
    assert lib.sa_coo_count(None, L.SA_F32, 16, None, None, None) == L.SA_ERR_ARG
    assert lib.sa_coo_decode(None, None, L.SA_F32, 4, 16, None, None, None) == L.SA_ERR_ARG


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_coo_scratch_bytes": "int sa_coo_scratch_bytes(uint64_t n, int x_type);",
        "sa_coo_count": "int sa_coo_count(const void* x, int x_type, uint64_t n, void* scratch, void* nnz_out, "
                        "void* stream);",
        "sa_coo_fill": "int sa_coo_fill(const void* x, int x_type, uint64_t n, const void* scratch, void* index_out, "
                       "void* data_out, uint64_t cap, void* flag, void* stream);",
        "sa_coo_decode": "int sa_coo_decode(const void* index, const void* data, int x_type, uint64_t nnz, "
                         "uint64_t n, void* dense_out, void* flag, void* stream);",
        "sa_coo_axpy": "int sa_coo_axpy(const void* index, const void* data, int x_type, uint64_t nnz, double w, "
                       "void* acc, int acc_type, uint64_t n, void* flag, void* stream);",
        "sa_coo_finish": "int sa_coo_finish(void* acc, int acc_type, uint64_t n, double divisor, void* stream);",
    }
    assert set(want) == set(ENTRIES)
    check_entries(want, (("SA_COO_BAD_RANGE", L.SA_COO_BAD_RANGE), ("SA_COO_BAD_ORDER", L.SA_COO_BAD_ORDER),
                         ("SA_COO_BAD_COUNT", L.SA_COO_BAD_COUNT)), "u")


def test_the_wrappers_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    from sfl_amd import kernels as K

    x = torch.ones(8)
    words = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="device-resident"):
        K.coo_count(x, words, words)
    with pytest.raises(ValueError, match="device-resident"):
        K.coo_finish(x, 2.0)
    with pytest.raises(TypeError):
        K.coo_scratch_bytes(16, torch.int64)
