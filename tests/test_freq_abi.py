"""The sa_freq_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, and what can be refused or finished
before any launch is."""
import ctypes as C

from abi_header import header

from sfl_amd import _lib as L

P16, ODD = C.c_void_p(0x1000), C.c_void_p(0x1004)  # never dereferenced: no call below launches
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double*": C.c_void_p,
         "void* const*": C.POINTER(C.c_void_p)}
PROTOS = {
    "sa_freq_scratch_bytes": "int sa_freq_scratch_bytes(uint64_t rows, uint64_t cols, int n_clients, int x_type);",
    "sa_freq_features": "int sa_freq_features(const void* const* w, int n_clients, int x_type, uint64_t rows, "
                        "uint64_t cols, void* scratch, double* feats_out, void* stream);",
    "sa_freq_gram": "int sa_freq_gram(const double* feats, int n_clients, uint64_t len, double* out, void* stream);",
}


def test_the_header_declares_what_the_binding_binds():
    flat = " ".join(header().split())
    lib = L.lib()
    for name, proto in PROTOS.items():
        assert name in L.EXPORTED and proto in flat, name
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        types = [KINDS[p.replace("const ", "", 1).rsplit(" ", 1)[0]] for p in params]
        assert list(getattr(lib, name).argtypes) == types, name
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_sizes_empty_calls_and_refusals():
    lib = L.lib()
    w = (C.c_void_p * 2)(P16.value, P16.value)

    def features(w=w, c=2, xt=L.SA_F32, rows=10, cols=64, scratch=P16, out=P16):
        return lib.sa_freq_features(w, c, xt, rows, cols, scratch, out, None)

    def refused(rc, word, code=L.SA_ERR_ARG):
        assert rc == code and word.encode() in lib.sa_last_error(), lib.sa_last_error()

    # A (5 x 10), B (19 x 64) and six clients' 19 x 10 first products, in doubles; (65, 130): hk = 32, wk = 49
    assert lib.sa_freq_scratch_bytes(10, 64, 6, L.SA_F64) == 8 * (5 * 10 + 19 * 64 + 6 * 19 * 10)
    assert lib.sa_freq_scratch_bytes(65, 130, 1, L.SA_F32) == 8 * (32 * 65 + 49 * 130 + 49 * 65)
    assert features(w=None, c=0, scratch=None, out=None) == L.SA_OK  # nothing to do: no pointer is looked at
    assert lib.sa_freq_gram(None, 0, 8, None, None) == L.SA_OK
    refused(lib.sa_freq_scratch_bytes(40000, 40000, 16, L.SA_F32), "above 2^31 - 1", L.SA_ERR_UNSUPPORTED)
    refused(features(rows=40000, cols=40000, c=2), "above 2^31 - 1", L.SA_ERR_UNSUPPORTED)
    refused(features(rows=1), "at least 2")
    refused(features(cols=2**24), "2^24")
    refused(features(xt=L.SA_I64), "SA_F32 or SA_F64")
    refused(features(c=17), "0..16")
    refused(features(w=None), "w, scratch and feats_out are required")
    refused(features(scratch=ODD), "aligned")
    refused(features(w=(C.c_void_p * 2)(P16.value, 0)), "client 1's w")
    refused(features(w=(C.c_void_p * 2)(0x1002, P16.value)), "client 0's w")
    refused(lib.sa_freq_gram(P16, 17, 8, P16, None), "0..16")
    refused(lib.sa_freq_gram(P16, 2, 2**32, P16, None), "2^32")
    refused(lib.sa_freq_gram(None, 2, 8, P16, None), "feats and out are required")
    refused(lib.sa_freq_gram(P16, 2, 8, ODD, None), "aligned")
