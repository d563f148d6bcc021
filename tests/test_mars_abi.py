"""The sa_mars_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, and what can be refused or finished
before any launch is."""
import ctypes as C
import re

from abi_header import header

from sfl_amd import _lib as L

P16, ODD = C.c_void_p(0x1000), C.c_void_p(0x1002)  # never dereferenced: no call below launches
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double*": C.c_void_p,
         "void* const*": C.POINTER(C.c_void_p)}
PROTOS = {
    "sa_mars_sigma": "int sa_mars_sigma(const void* const* w, int n_clients, int x_type, uint64_t n_mat, uint64_t rows, "
                     "uint64_t cols, const void* const* bn_w, const void* const* bn_var, uint64_t n_bn, double* out, "
                     "void* stream);",
    "sa_mars_bn": "int sa_mars_bn(const void* const* bn_w, const void* const* bn_var, int n_clients, int x_type, "
                  "uint64_t n_bn, double* out, void* stream);",
}


def _table(*ptrs):
    return (C.c_void_p * len(ptrs))(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])


def test_the_header_declares_what_the_binding_binds():
    hdr = header()
    flat = " ".join(hdr.split())
    lib = L.lib()
    for name, proto in PROTOS.items():
        assert name in L.EXPORTED and proto in flat, name
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        types = [KINDS[p.replace("const ", "", 1).rsplit(" ", 1)[0]] for p in params]
        assert list(getattr(lib, name).argtypes) == types, name
    assert re.search(r"#define SA_MARS_MAX_P %d\b" % L.SA_MARS_MAX_P, hdr) and L.SA_MARS_MAX_P == 32
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_empty_calls_touch_nothing_and_bad_ones_are_refused():
    lib = L.lib()
    w = _table(P16, P16)

    def sigma(w=w, c=2, xt=L.SA_F32, n_mat=4, rows=8, cols=9, bw=None, bv=None, n_bn=0, out=P16):
        return lib.sa_mars_sigma(w, c, xt, n_mat, rows, cols, bw, bv, n_bn, out, None)

    def refused(rc, word, code=L.SA_ERR_ARG):
        assert rc == code and word.encode() in lib.sa_last_error(), lib.sa_last_error()

    # nothing to do: no pointer is looked at
    assert sigma(w=None, c=0, out=None) == L.SA_OK
    assert sigma(w=None, n_mat=0, out=None) == L.SA_OK
    assert lib.sa_mars_bn(None, None, 0, L.SA_F64, 8, None, None) == L.SA_OK
    assert lib.sa_mars_bn(None, None, 2, L.SA_F64, 0, None, None) == L.SA_OK
    refused(sigma(rows=33, cols=40), "SA_MARS_MAX_P", L.SA_ERR_UNSUPPORTED)
    refused(sigma(rows=0), "SA_MARS_MAX_P", L.SA_ERR_UNSUPPORTED)
    refused(sigma(xt=L.SA_I64), "SA_F32 or SA_F64")
    refused(sigma(c=17), "0..16")
    refused(sigma(c=-1), "0..16")
    refused(sigma(n_mat=2**24), "2^24")
    refused(sigma(rows=2**24, cols=3), "2^24")
    refused(sigma(w=None), "w is required")
    refused(sigma(out=None), "out is required")
    refused(sigma(out=C.c_void_p(0x1004)), "aligned")
    refused(sigma(w=_table(P16, 0)), "client 1's w")
    refused(sigma(w=_table(ODD, P16)), "client 0's w")
    refused(sigma(n_bn=4), "bn_w and bn_var are required")
    refused(sigma(bw=w, bv=_table(P16, ODD), n_bn=4), "client 1's bn_var")
    refused(lib.sa_mars_bn(w, None, 2, L.SA_F32, 8, P16, None), "bn_var is required")
    refused(lib.sa_mars_bn(_table(0, P16), w, 2, L.SA_F32, 8, P16, None), "client 0's bn_w")
    refused(lib.sa_mars_bn(w, w, 2, 7, 8, P16, None), "SA_F32 or SA_F64")
    refused(lib.sa_mars_bn(w, w, 2, L.SA_F32, 2**32, P16, None), "2^32")
    refused(lib.sa_mars_bn(w, w, 2, L.SA_F32, 8, None, None), "out is required")
