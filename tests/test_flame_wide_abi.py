"""The sa_flame_*_wide entries (17 to 64 clients) without a GPU: the library
exports them, the header declares what sfl_amd/_lib.py binds, the scratch's
size is the statistics pass's grid of partials, and the arguments that can be
refused before any launch are refused."""
import ctypes as C
import re

import pytest
from abi_header import header

from sfl_amd import _lib as L

ENTRIES = ("sa_flame_wide_scratch_bytes", "sa_flame_stats_wide", "sa_flame_combine_wide")
# addresses that are never dereferenced: every call below is refused before any launch
P16, P8, ODD = C.c_void_p(0x1000), C.c_void_p(0x2008), C.c_void_p(0x1002)
# the prototypes' parameter types as the binding states them (host tables are typed pointers)
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double": C.c_double,
         "void* const*": C.POINTER(C.c_void_p)}
NC = 17  # the smallest client count the entries take


def _table(*ptrs):
    return (C.c_void_p * len(ptrs))(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])


def _doubles(*v):
    return (C.c_double * len(v))(*v)


def _refused(rc, word):
    assert rc == L.SA_ERR_ARG
    assert word.encode() in L.lib().sa_last_error(), L.lib().sa_last_error()


def _with(k, p, n=NC):
    """A table of ``n`` good addresses with ``p`` for client ``k``."""
    return _table(*[p if i == k else P16 for i in range(n)])


def test_the_library_exports_the_three_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.sa_abi_version() == 3  # the entries are additive
    assert L.SA_FLAME_MAX_CLIENTS == 16 and L.SA_FLAME_WIDE_MAX_CLIENTS == 64


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_flame_wide_scratch_bytes": ("int sa_flame_wide_scratch_bytes(uint64_t n, int n_clients, int x_type);", {}),
        "sa_flame_stats_wide": ("int sa_flame_stats_wide(const void* const* x, int n_clients, int x_type, uint64_t n, "
                                "void* median_out, void* scratch, double* stats, int accumulate, void* stream);",
                                {"stats": C.c_void_p}),  # device memory: an address
        "sa_flame_combine_wide": ("int sa_flame_combine_wide(const void* const* x, const double* scale, "
                                  "const double* weight, int n_clients, int x_type, uint64_t n, const void* median, "
                                  "double divisor, double* out, void* stream);",
                                  {"scale": C.POINTER(C.c_double), "weight": C.POINTER(C.c_double),
                                   "out": C.c_void_p}),
    }
    assert set(want) == set(ENTRIES)
    hdr = header()
    flat = " ".join(hdr.split())
    lib = L.lib()
    for name, (proto, typed) in want.items():
        assert proto in flat, name
        types = []
        for p in proto[proto.index("(") + 1:proto.rindex(")")].split(", "):
            kind, arg = p.replace("const ", "", 1).rsplit(" ", 1)
            types.append(typed[arg] if arg in typed else KINDS[kind])
        assert list(getattr(lib, name).argtypes) == types, name
    assert re.search(r"#define SA_FLAME_WIDE_MAX_CLIENTS %d\b" % L.SA_FLAME_WIDE_MAX_CLIENTS, hdr)
    assert re.search(r"#define SA_ABI_VERSION 3\b", hdr)


def _scratch_bytes(n, c):
    """sa_flame_wide.hip's stat_grid and partial_count: a block's partial is the
    Gram tiles of the padded client count as the matrix instruction leaves
    them (256 values a tile), then the padded clients' N."""
    tiles = (n + 127) // 128
    per_block = (tiles + 511) // 512
    blocks = (tiles + per_block - 1) // per_block if per_block else 0
    cp = 32 if c <= 32 else 64
    return blocks * ((cp // 16) * (cp // 16 + 1) // 2 * 256 + cp) * 8


def test_scratch_bytes_validates_without_a_gpu():
    lib = L.lib()
    _refused(lib.sa_flame_wide_scratch_bytes(2**32, 32, L.SA_F32), "2^32")
    _refused(lib.sa_flame_wide_scratch_bytes(16, 32, L.SA_I64), "SA_F32 or SA_F64")
    for c in (-1, 0, 1, 16, 65, 1000):
        _refused(lib.sa_flame_wide_scratch_bytes(16, c, L.SA_F32), "n_clients must be in 17..64")
    assert b"(SA_FLAME_WIDE_MAX_CLIENTS; 1..16: the sa_flame_* entries)" in lib.sa_last_error()
    assert _scratch_bytes(1, 17) == 800 * 8 and _scratch_bytes(512 * 128 + 1, 64) == 257 * 2624 * 8
    # a block of partials per tile of 128 elements up to 512 blocks, then whole tiles a block; none for n == 0
    for n in (0, 1, 128, 129, 512 * 128, 512 * 128 + 1, 3 * 512 * 128 + 5, 2**32 - 1):
        for c in (17, 32, 33, 64):
            for xt in (L.SA_F32, L.SA_F64):
                assert lib.sa_flame_wide_scratch_bytes(n, c, xt) == _scratch_bytes(n, c), (n, c)


def test_bad_types_sizes_and_client_counts_are_refused_before_any_launch():
    lib = L.lib()
    x, s, w = _with(0, P16), _doubles(*[1.0] * NC), _doubles(*[1.0] * NC)
    for n, xt, word in ((2**32, L.SA_F32, "2^32"), (16, L.SA_I64, "SA_F32 or SA_F64"), (16, 7, "SA_F32 or SA_F64")):
        _refused(lib.sa_flame_stats_wide(x, NC, xt, n, P16, P8, P8, 0, None), word)
        _refused(lib.sa_flame_combine_wide(x, s, w, NC, xt, n, P16, 2.0, P8, None), word)
    for c in (-3, 0, 16, 65):
        _refused(lib.sa_flame_stats_wide(x, c, L.SA_F32, 16, P16, P8, P8, 0, None), "n_clients must be in 17..64")
        _refused(lib.sa_flame_combine_wide(x, s, w, c, L.SA_F32, 16, P16, 2.0, P8, None),
                 "n_clients must be in 17..64")
    # the element type is judged before the size, the size before the client count
    _refused(lib.sa_flame_stats_wide(x, 16, 7, 2**32, P16, P8, P8, 0, None), "SA_F32 or SA_F64")
    _refused(lib.sa_flame_combine_wide(x, s, w, 16, L.SA_F32, 2**32, P16, 2.0, P8, None), "2^32")


def test_null_and_misaligned_pointers_are_refused():
    lib = L.lib()
    x, s, w = _with(0, P16), _doubles(*[1.0] * NC), _doubles(*[1.0] * NC)
    _refused(lib.sa_flame_stats_wide(None, NC, L.SA_F32, 16, P16, P8, P8, 0, None), "x, median_out and scratch")
    _refused(lib.sa_flame_stats_wide(x, NC, L.SA_F32, 16, None, P8, P8, 0, None), "x, median_out and scratch")
    _refused(lib.sa_flame_stats_wide(x, NC, L.SA_F32, 16, P16, None, P8, 0, None), "x, median_out and scratch")
    _refused(lib.sa_flame_stats_wide(x, NC, L.SA_F32, 16, P16, P8, None, 0, None), "stats is required")
    _refused(lib.sa_flame_stats_wide(x, NC, L.SA_F32, 0, P16, P8, None, 1, None), "stats is required")  # even for n == 0
    _refused(lib.sa_flame_stats_wide(None, NC, L.SA_F32, 16, P16, P8, None, 0, None), "stats is required")  # stats first
    _refused(lib.sa_flame_stats_wide(_with(16, 0), NC, L.SA_F32, 16, P16, P8, P8, 0, None), "client 16's tensor")
    _refused(lib.sa_flame_stats_wide(_with(0, ODD), NC, L.SA_F32, 16, P16, P8, P8, 0, None), "client 0's tensor")
    _refused(lib.sa_flame_stats_wide(_with(5, C.c_void_p(0x1004)), NC, L.SA_F64, 16, P16, P8, P8, 0, None),
             "client 5's tensor is required, element-aligned")
    _refused(lib.sa_flame_stats_wide(_with(40, 0, 64), 64, L.SA_F64, 16, P16, P8, P8, 0, None), "client 40's tensor")
    _refused(lib.sa_flame_stats_wide(x, NC, L.SA_F32, 16, ODD, P8, P8, 0, None), "element-aligned median_out")
    _refused(lib.sa_flame_stats_wide(x, NC, L.SA_F32, 16, P16, C.c_void_p(0x2004), P8, 0, None), "8-byte aligned scratch")
    _refused(lib.sa_flame_stats_wide(x, NC, L.SA_F32, 16, P16, P8, C.c_void_p(0x2004), 0, None), "8-byte aligned")
    # the joint check comes before the table's walk
    _refused(lib.sa_flame_stats_wide(_with(0, 0), NC, L.SA_F32, 16, None, P8, P8, 0, None), "x, median_out and scratch")
    _refused(lib.sa_flame_combine_wide(None, s, w, NC, L.SA_F32, 16, P16, 2.0, P8, None), "x, scale and weight")
    _refused(lib.sa_flame_combine_wide(x, None, w, NC, L.SA_F32, 16, P16, 2.0, P8, None), "x, scale and weight")
    _refused(lib.sa_flame_combine_wide(x, s, None, NC, L.SA_F32, 16, P16, 2.0, P8, None), "x, scale and weight")
    _refused(lib.sa_flame_combine_wide(x, s, w, NC, L.SA_F32, 16, None, 2.0, P8, None), "median and out are required")
    _refused(lib.sa_flame_combine_wide(x, s, w, NC, L.SA_F32, 16, P16, 2.0, None, None), "median and out are required")
    _refused(lib.sa_flame_combine_wide(_with(16, 0), s, w, NC, L.SA_F32, 16, P16, 2.0, P8, None), "client 16's tensor")
    _refused(lib.sa_flame_combine_wide(_with(3, ODD), s, w, NC, L.SA_F32, 16, P16, 2.0, P8, None), "client 3's tensor")
    _refused(lib.sa_flame_combine_wide(x, s, w, NC, L.SA_F32, 16, ODD, 2.0, P8, None), "element-aligned median")
    _refused(lib.sa_flame_combine_wide(x, s, w, NC, L.SA_F32, 16, P16, 2.0, C.c_void_p(0x2004), None), "aligned out")
    # a client's pointer is judged before median and out
    _refused(lib.sa_flame_combine_wide(_with(3, 0), s, w, NC, L.SA_F32, 16, None, 2.0, None, None), "client 3's tensor")


def test_a_dropped_clients_pointer_is_not_looked_at():
    lib = L.lib()
    nan = float("nan")
    x, s = _with(0, P16), _doubles(*[1.0] * NC)
    # a NaN weight drops a client: every client dropped is refused, also for n == 0 and before median and out
    _refused(lib.sa_flame_combine_wide(x, s, _doubles(*[nan] * NC), NC, L.SA_F32, 16, P16, 2.0, P8, None), "dropped")
    _refused(lib.sa_flame_combine_wide(x, s, _doubles(*[nan] * NC), NC, L.SA_F32, 0, None, 2.0, None, None), "dropped")
    # client 4 is dropped and its null pointer passes; client 5's, kept, is what is refused
    w = _doubles(*[nan if i == 4 else 1.0 for i in range(NC)])
    bad = _table(*[0 if i in (4, 5) else P16 for i in range(NC)])
    _refused(lib.sa_flame_combine_wide(bad, s, w, NC, L.SA_F32, 16, P16, 2.0, P8, None), "client 5's tensor")
    _refused(lib.sa_flame_combine_wide(_with(4, ODD), s, w, NC, L.SA_F32, 16, None, 2.0, P8, None),
             "median and out are required")
    assert lib.sa_flame_combine_wide(_with(4, 0), s, w, NC, L.SA_F32, 0, None, 1.0, None, None) == L.SA_OK


def test_empty_calls_launch_nothing():
    lib = L.lib()
    ones = _doubles(*[1.0] * NC)
    # n == 0: no pointer of a client is looked at; with accumulate there is nothing to add to stats
    assert lib.sa_flame_combine_wide(_with(0, 0), ones, ones, NC, L.SA_F64, 0, None, 2.0, None, None) == L.SA_OK
    assert lib.sa_flame_stats_wide(None, NC, L.SA_F32, 0, None, None, P8, 1, None) == L.SA_OK
    assert lib.sa_flame_stats_wide(_with(0, ODD), 64, L.SA_F64, 0, ODD, ODD, P8, 1, None) == L.SA_OK


def test_the_wrappers_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    from sfl_amd import kernels as K

    x, out = torch.ones(8), torch.zeros(8, dtype=torch.float64)
    with pytest.raises(ValueError, match="device-resident"):
        K.flame_stats_wide([x] * NC, torch.empty(8), torch.empty(64, dtype=torch.uint8),
                           torch.zeros(K.flame_stat_count(NC), dtype=torch.float64))
    with pytest.raises(ValueError, match="device-resident"):
        K.flame_combine_wide([x] * NC, [1.0] * NC, [1.0] * NC, [True] * NC, x, 2.0, out)
    with pytest.raises(TypeError):
        K.flame_wide_scratch_bytes(16, NC, torch.int64)
    assert K.flame_wide_scratch_bytes(16, NC, torch.float32) == 800 * 8
    assert K.flame_wide_scratch_bytes(129, 33, torch.float64) == 2 * 2624 * 8
