"""The sa_bin_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, what can be refused or finished before any
launch is, and the launch geometry keeps its promises."""
import ctypes as C

import pytest
import torch
from abi_header import header

from sfl_amd import _lib as L
from sfl_amd import kernels as K

P16, ODD = C.c_void_p(0x1000), C.c_void_p(0x1002)  # never dereferenced: no call below launches
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double*": C.c_void_p, "int64_t*": C.c_void_p,
         "int*": C.POINTER(C.c_int)}
PROTOS = {
    "sa_bin_geometry": "int sa_bin_geometry(int q, uint64_t n_features, int x_type, int* out5);",
    "sa_bin_range": "int sa_bin_range(const void* x, int x_type, uint64_t rows, uint64_t n_features, "
                    "const double* abnormal, int n_abnormal, void* out, void* stream);",
    "sa_bin_ranks": "int sa_bin_ranks(const void* x, int x_type, uint64_t rows, uint64_t n_features, "
                    "const double* queries, int q, const double* abnormal, int n_abnormal, int64_t* ranks_out, "
                    "void* stream);",
}
HOST_ARRAYS = {("sa_bin_range", 4), ("sa_bin_ranks", 6)}  # abnormal: read by the call, bound as double*
LDS_BUDGET = 65536


def test_the_header_declares_what_the_binding_binds():
    hdr = header()
    flat = " ".join(hdr.split())
    lib = L.lib()
    for name, proto in PROTOS.items():
        assert name in L.EXPORTED and proto in flat, name
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        types = [C.POINTER(C.c_double) if (name, i) in HOST_ARRAYS else
                 KINDS[p.replace("const ", "", 1).rsplit(" ", 1)[0]] for i, p in enumerate(params)]
        assert list(getattr(lib, name).argtypes) == types, name
    for word, value in (("SA_BIN_MAX_Q", 255), ("SA_BIN_REG_MAX_Q", 16), ("SA_BIN_MAX_ABNORMAL", 4)):
        assert f"#define {word} {value}" in hdr and getattr(L, word) == value
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_empty_calls_and_refusals():
    lib = L.lib()
    two = (C.c_double * 4)(1.0, 2.0)

    def rng(x=P16, xt=L.SA_F32, rows=10, nf=3, ab=two, na=2, out=P16):
        return lib.sa_bin_range(x, xt, rows, nf, ab, na, out, None)

    def ranks(x=P16, xt=L.SA_F32, rows=10, nf=3, q=P16, nq=10, ab=None, na=0, out=P16):
        return lib.sa_bin_ranks(x, xt, rows, nf, q, nq, ab, na, out, None)

    def refused(rc, word):
        assert rc == L.SA_ERR_ARG and word.encode() in lib.sa_last_error(), lib.sa_last_error()

    assert rng(x=None, nf=0, out=None) == L.SA_OK and ranks(x=None, nf=0, q=None, out=None) == L.SA_OK
    refused(rng(xt=L.SA_I64), "SA_F32 or SA_F64")
    refused(rng(rows=2 ** 40), "rows must be below 2^40")
    refused(ranks(nf=2 ** 16), "n_features below 2^16")
    refused(rng(na=5), "n_abnormal must be in 0..4")
    refused(ranks(ab=None, na=1), "n_abnormal must be in 0..4")
    refused(rng(x=None), "x and out are required")
    refused(rng(out=ODD), "aligned")
    for nq in (0, 256):
        refused(ranks(nq=nq), "q must be in 1..255")
    refused(ranks(q=None), "x, queries and ranks_out are required")
    refused(ranks(xt=L.SA_F64, x=C.c_void_p(0x1004)), "aligned")
    refused(ranks(out=None), "x, queries and ranks_out are required")
    refused(lib.sa_bin_geometry(10, 0, L.SA_F32, (C.c_int * 5)()), "at least one feature")
    refused(lib.sa_bin_geometry(10, 3, L.SA_F32, None), "out5 is required")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n_features", [1, 33, 64, 65])
@pytest.mark.parametrize("q", [1, 4, 5, 8, 9, 16, 17, 32, 255])
def test_geometry(q, n_features, dtype):
    """Registers up to 16 query points and LDS above; the padding admits every
    query point; a group is at most a wave wide, fits the LDS budget and the
    groups cover the features."""
    esz = 4 if dtype == torch.float32 else 8
    form, qp, fg, lds, groups = K.bin_geometry(q, n_features, dtype)
    assert form == (0 if q <= 16 else 1) and 1 <= fg <= min(64, n_features) and groups == -(-n_features // fg)
    if form == 0:
        assert qp == (4 if q <= 4 else 8 if q <= 8 else 16) and fg == min(64, n_features) and lds == 64 * qp * 4
    else:
        assert qp == 1 << q.bit_length() and qp > q  # qp - 1 >= q entries are searched
        assert lds == fg * qp * (esz + 4) <= LDS_BUDGET
        assert fg == min(64, n_features, LDS_BUDGET // (qp * (esz + 4)))
    if q == 255:
        assert fg == min(n_features, 32 if esz == 4 else 21)
