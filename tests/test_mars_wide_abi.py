"""sa_mars_wide_scratch_bytes / sa_mars_sigma_wide without a GPU: the library
exports them, the header declares what sfl_amd/_lib.py binds, and what can be
refused or finished before any launch is."""
import ctypes as C
import re

from abi_header import header

from sfl_amd import _lib as L

P16, ODD = C.c_void_p(0x1000), C.c_void_p(0x1002)  # never dereferenced: no call below launches
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double*": C.c_void_p,
         "void* const*": C.POINTER(C.c_void_p)}
PROTOS = {
    "sa_mars_wide_scratch_bytes": "int sa_mars_wide_scratch_bytes(int n_clients, uint64_t n_mat, uint64_t rows, "
                                  "uint64_t cols);",
    "sa_mars_sigma_wide": "int sa_mars_sigma_wide(const void* const* w, int n_clients, int x_type, uint64_t n_mat, "
                          "uint64_t rows, uint64_t cols, const void* const* bn_w, const void* const* bn_var, "
                          "uint64_t n_bn, void* scratch, double* out, void* stream);",
}


def test_the_header_declares_what_the_binding_binds():
    hdr = header()
    flat = " ".join(hdr.split())
    lib = L.lib()
    for name, proto in PROTOS.items():
        assert name in L.EXPORTED and proto in flat, name
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        types = [KINDS[p.replace("const ", "", 1).rsplit(" ", 1)[0]] for p in params]
        assert list(getattr(lib, name).argtypes) == types, name
    assert re.search(r"#define SA_MARS_WIDE_MAX_P %d\b" % L.SA_MARS_WIDE_MAX_P, hdr) and L.SA_MARS_WIDE_MAX_P == 512
    assert lib.sa_abi_version() == 3  # the entries are additive
    assert lib.sa_mars_wide_scratch_bytes(2, 3, 40, 48) == 2 * 3 * 40 * 40 * 8


def test_empty_calls_touch_nothing_and_bad_ones_are_refused():
    lib = L.lib()
    w = (C.c_void_p * 2)(P16.value, P16.value)

    def sigma(w=w, c=2, n_mat=4, rows=40, cols=48, bw=None, n_bn=0, scratch=P16, out=P16):
        return lib.sa_mars_sigma_wide(w, c, L.SA_F32, n_mat, rows, cols, bw, None, n_bn, scratch, out, None)

    def refused(rc, word, code=L.SA_ERR_ARG):
        assert rc == code and word.encode() in lib.sa_last_error(), lib.sa_last_error()

    # nothing to do: no pointer is looked at
    assert sigma(w=None, c=0, scratch=None, out=None) == L.SA_OK
    assert sigma(w=None, n_mat=0, scratch=None, out=None) == L.SA_OK
    refused(sigma(rows=0), "SA_MARS_WIDE_MAX_P", L.SA_ERR_UNSUPPORTED)
    refused(sigma(rows=513, cols=600), "SA_MARS_WIDE_MAX_P", L.SA_ERR_UNSUPPORTED)
    refused(lib.sa_mars_wide_scratch_bytes(2, 3, 513, 600), "SA_MARS_WIDE_MAX_P", L.SA_ERR_UNSUPPORTED)
    refused(lib.sa_mars_wide_scratch_bytes(16, 600, 512, 512), "2^31 - 1", L.SA_ERR_UNSUPPORTED)
    refused(sigma(c=17), "0..16")
    refused(sigma(scratch=None), "scratch and out are required")
    refused(sigma(out=None), "scratch and out are required")
    refused(sigma(scratch=C.c_void_p(0x1004)), "aligned")
    refused(sigma(n_bn=4), "bn_w and bn_var are required")
    refused(sigma(bw=w, n_bn=4), "bn_w and bn_var are required")
