"""The sa_stc and sa_scr entries without a GPU: the library exports them and
the header declares what sfl_amd/_lib.py binds.  What they refuse before any
launch is in test_compress_abi.py."""
from abi_header import check_entries

from sfl_amd import _lib as L

ENTRIES = ("sa_stc_scratch_bytes", "sa_stc", "sa_scr_scratch_bytes", "sa_scr")


def test_the_library_exports_the_four_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_stc_scratch_bytes": "int sa_stc_scratch_bytes(uint64_t n, int x_type);",
        "sa_stc": "int sa_stc(const void* a, const void* b, const void* r, int x_type, uint64_t n, uint64_t mask_num, "
                  "void* sparse_out, void* res_out, void* acc_inout, void* mu_out, void* scratch, void* stream);",
        "sa_scr_scratch_bytes": "int sa_scr_scratch_bytes(uint64_t rows, uint64_t cols, uint64_t inner, int x_type);",
        "sa_scr": "int sa_scr(const void* a, const void* b, const void* r, int x_type, uint64_t rows, uint64_t cols, "
                  "uint64_t inner, double threshold, void* sparse_out, void* res_out, void* stats_out, void* scratch, "
                  "void* stream);",
    }
    assert set(want) == set(ENTRIES)
    check_entries(want)
