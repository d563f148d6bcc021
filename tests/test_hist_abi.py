"""The sa_hist_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, what can be refused or finished before
any launch is, and the launch geometry keeps its promises."""
import ctypes as C

import pytest
from abi_header import header

from sfl_amd import _lib as L
from sfl_amd import kernels as K

P16, ODD = C.c_void_p(0x1000), C.c_void_p(0x1002)  # never dereferenced: no call below launches
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double*": C.c_void_p, "int32_t*": C.c_void_p,
         "uint8_t*": C.c_void_p, "int*": C.POINTER(C.c_int)}
PROTOS = {
    "sa_hist_scratch_bytes": "int sa_hist_scratch_bytes(uint64_t n_nodes, uint64_t n_features, int bmax);",
    "sa_hist_geometry": "int sa_hist_geometry(int bmax, int n_nodes, uint64_t n_features, int* out4);",
    "sa_hist_codes": "int sa_hist_codes(const void* x, int x_type, uint64_t rows, uint64_t n_features, "
                     "const double* splits, const int32_t* offsets, int bmax, uint8_t* codes_out, void* stream);",
    "sa_hist_build": "int sa_hist_build(const uint8_t* codes, uint64_t rows, uint64_t n_features, int bmax, "
                     "const int32_t* node_of_row, int n_nodes, const void* grad, const void* hess, int g_type, "
                     "int k_grad, int k_hess, void* scratch, void* stream);",
    "sa_hist_finish": "int sa_hist_finish(const void* scratch, int n_nodes, uint64_t n_features, int bmax, "
                      "const int32_t* n_bins, int k_grad, int k_hess, int use_missing, double* out, void* stream);",
}
LDS_BUDGET = 65536  # two blocks resident in a CU's 160 KiB


def test_the_header_declares_what_the_binding_binds():
    hdr = header()
    flat = " ".join(hdr.split())
    lib = L.lib()
    for name, proto in PROTOS.items():
        assert name in L.EXPORTED and proto in flat, name
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        types = [KINDS[p.replace("const ", "", 1).rsplit(" ", 1)[0]] for p in params]
        assert list(getattr(lib, name).argtypes) == types, name
    assert "#define SA_HIST_MAX_BINS 255" in hdr and L.SA_HIST_MAX_BINS == 255
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_sizes_empty_calls_and_refusals():
    lib = L.lib()

    def codes(x=P16, xt=L.SA_F32, rows=10, nf=3, splits=P16, offs=P16, bmax=4, out=P16):
        return lib.sa_hist_codes(x, xt, rows, nf, splits, offs, bmax, out, None)

    def build(codes=P16, rows=10, nf=3, bmax=4, node=P16, n=2, g=P16, h=P16, gt=L.SA_F32, kg=0, kh=0, scratch=P16):
        return lib.sa_hist_build(codes, rows, nf, bmax, node, n, g, h, gt, kg, kh, scratch, None)

    def finish(scratch=P16, n=2, nf=3, bmax=4, nb=P16, kg=0, kh=0, miss=0, out=P16):
        return lib.sa_hist_finish(scratch, n, nf, bmax, nb, kg, kh, miss, out, None)

    def refused(rc, word, code=L.SA_ERR_ARG):
        assert rc == code and word.encode() in lib.sa_last_error(), lib.sa_last_error()

    # (G, H, N) = 8 + 8 + 4 bytes a (slot, feature, code): 2 x 3 x 2 entries; 1 x 1 x 1 rounded up to 8
    assert lib.sa_hist_scratch_bytes(2, 3, 1) == 240
    assert lib.sa_hist_scratch_bytes(1, 1, 0) == 24
    assert lib.sa_hist_scratch_bytes(20, 64, 255) == 20 * 64 * 256 * 20
    assert codes(x=None, rows=0, splits=None, offs=None, out=None) == L.SA_OK  # nothing to do: no pointer is looked at
    assert build(codes=None, node=None, n=0, g=None, h=None, scratch=None) == L.SA_OK
    assert finish(scratch=None, nf=0, nb=None, out=None) == L.SA_OK
    refused(lib.sa_hist_scratch_bytes(2 ** 20, 2 ** 10, 255), "above 2^31 - 1", L.SA_ERR_UNSUPPORTED)
    refused(build(n=2 ** 20, nf=2 ** 10, bmax=255), "above 2^31 - 1", L.SA_ERR_UNSUPPORTED)
    refused(lib.sa_hist_scratch_bytes(1, 1, 256), "bmax must be in 0..255")
    refused(lib.sa_hist_scratch_bytes(2 ** 24, 1, 1), "n_nodes must be below 2^24")
    refused(lib.sa_hist_geometry(4, 0, 3, (C.c_int * 4)()), "at least one node")
    refused(codes(xt=L.SA_I64), "SA_F32 or SA_F64")
    refused(codes(rows=2 ** 31), "rows must be below 2^31")
    refused(codes(bmax=-1), "bmax must be in 0..255")
    refused(codes(x=None), "x, splits, offsets and codes_out are required")
    refused(codes(offs=ODD), "aligned")
    refused(build(gt=L.SA_I64), "the gradients' type must be SA_F32 or SA_F64")
    refused(build(n=-1), "n_nodes must be below 2^24")
    refused(build(kg=3000), "k_grad must be in -2100..2100")
    refused(build(kh=-3000), "k_hess must be in -2100..2100")
    refused(build(scratch=None), "scratch is required")
    refused(build(g=None), "codes, node_of_row, grad and hess are required")
    refused(build(gt=L.SA_F64, h=C.c_void_p(0x1004)), "aligned")
    refused(finish(nb=None), "scratch, n_bins and out are required")
    refused(finish(out=ODD), "aligned")
    refused(finish(kg=3000), "k_grad must be in -2100..2100")


@pytest.mark.parametrize("bmax", [1, 32, 255])
@pytest.mark.parametrize("n_nodes", [1, 20, 21, 64])
@pytest.mark.parametrize("n_features", [1, 5, 64])
def test_geometry(bmax, n_nodes, n_features):
    """The feature group times the slots times the bins fits the LDS budget,
    and the launches cover every slot exactly once."""
    fg, slots, launches, lds = K.hist_geometry(bmax, n_nodes, n_features)
    assert fg in (4, 8, 16) and fg < n_features + 4 and slots >= 1
    assert lds == fg * slots * (bmax + 1) * 20 <= LDS_BUDGET
    covered = [s for first in range(0, n_nodes, slots) for s in range(first, min(first + slots, n_nodes))]
    assert covered == list(range(n_nodes)) and launches == len(range(0, n_nodes, slots))
    if bmax == 255:
        assert (fg, slots) == ((8, 1) if n_nodes == 1 and n_features > 4 else (4, min(3, n_nodes)))
