"""The sa_flame_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, and the arguments that can be refused
before any launch are refused."""
import ctypes as C
import os
import re

import pytest
from abi_header import ROOT, header

from sfl_amd import _lib as L

ENTRIES = ("sa_flame_scratch_bytes", "sa_flame_stats", "sa_flame_combine")
# addresses that are never dereferenced: every call below is refused before any launch
P16, P8, ODD = C.c_void_p(0x1000), C.c_void_p(0x2008), C.c_void_p(0x1002)
# the prototypes' parameter types as the binding states them (host tables are typed pointers)
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double": C.c_double,
         "void* const*": C.POINTER(C.c_void_p)}


def _table(*ptrs):
    return (C.c_void_p * len(ptrs))(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])


def _doubles(*v):
    return (C.c_double * len(v))(*v)


def _refused(rc, word):
    assert rc == L.SA_ERR_ARG
    assert word.encode() in L.lib().sa_last_error(), L.lib().sa_last_error()


def test_the_library_exports_the_three_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.sa_abi_version() == 3  # the entries are additive
    assert L.ABI_VERSION == 3 and L.SA_FLAME_MAX_CLIENTS == 16


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_flame_scratch_bytes": ("int sa_flame_scratch_bytes(uint64_t n, int n_clients, int x_type);", {}),
        "sa_flame_stats": ("int sa_flame_stats(const void* const* x, int n_clients, int x_type, uint64_t n, "
                           "void* median_out, void* scratch, double* stats, int accumulate, void* stream);",
                           {"stats": C.c_void_p}),  # device memory: an address
        "sa_flame_combine": ("int sa_flame_combine(const void* const* x, const double* scale, const double* weight, "
                             "int n_clients, int x_type, uint64_t n, const void* median, double divisor, double* out, "
                             "void* stream);",
                             {"scale": C.POINTER(C.c_double), "weight": C.POINTER(C.c_double), "out": C.c_void_p}),
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
    assert re.search(r"#define SA_FLAME_MAX_CLIENTS %d\b" % L.SA_FLAME_MAX_CLIENTS, hdr)
    assert re.search(r"#define SA_ABI_VERSION 3\b", hdr)


def test_the_header_cites_the_references_lines_for_every_entry():
    text = open(os.path.join(ROOT, "include", "sfl_sa.h")).read()
    block = text[text.index("FlameAggregator: the per-element work"):text.index("#define SA_FLAME_MAX_CLIENTS")]
    assert "agg_flame.py:27-203" in block
    stats = block[block.index("sa_flame_stats "):block.index("sa_flame_combine ")]
    combine = block[block.index("sa_flame_combine "):]
    assert len(re.findall(r":\s*\d+-\d+", stats)) >= 3 and "agg_flame.py" in stats
    assert re.search(r"agg_flame\.py:141-168", combine) and re.search(r":181-187", combine)


def test_scratch_bytes_validates_without_a_gpu():
    lib = L.lib()
    _refused(lib.sa_flame_scratch_bytes(2**32, 8, L.SA_F32), "2^32")
    _refused(lib.sa_flame_scratch_bytes(16, 8, L.SA_I64), "SA_F32 or SA_F64")
    for c in (-1, 0, 17, 1000):
        _refused(lib.sa_flame_scratch_bytes(16, c, L.SA_F32), "1..16")
    # one block of partials per 1,024 elements, at most 1,024 blocks; a block also for n == 0
    for n, c, blocks in ((0, 1, 1), (1, 3, 1), (1024, 8, 1), (1025, 8, 2), (2**20 + 1029, 16, 1024),
                         (2**32 - 1, 16, 1024)):
        for xt in (L.SA_F32, L.SA_F64):
            assert lib.sa_flame_scratch_bytes(n, c, xt) == blocks * (c * (c + 1) // 2 + c) * 8, (n, c)


def test_bad_types_sizes_and_client_counts_are_refused_before_any_launch():
    lib = L.lib()
    x, s, w = _table(P16, P16), _doubles(1.0, 1.0), _doubles(1.0, 1.0)
    for n, xt, word in ((2**32, L.SA_F32, "2^32"), (16, L.SA_I64, "SA_F32 or SA_F64"), (16, 7, "SA_F32 or SA_F64")):
        _refused(lib.sa_flame_stats(x, 2, xt, n, P16, P8, P8, 0, None), word)
        _refused(lib.sa_flame_combine(x, s, w, 2, xt, n, P16, 2.0, P8, None), word)
    for c in (-3, 0, 17):
        _refused(lib.sa_flame_stats(x, c, L.SA_F32, 16, P16, P8, P8, 0, None), "n_clients must be in 1..16")
        _refused(lib.sa_flame_combine(x, s, w, c, L.SA_F32, 16, P16, 2.0, P8, None), "n_clients must be in 1..16")


def test_null_and_misaligned_pointers_are_refused():
    lib = L.lib()
    x, s, w = _table(P16, P16), _doubles(1.0, 1.0), _doubles(1.0, 1.0)
    _refused(lib.sa_flame_stats(None, 2, L.SA_F32, 16, P16, P8, P8, 0, None), "required")
    _refused(lib.sa_flame_stats(x, 2, L.SA_F32, 16, None, P8, P8, 0, None), "required")
    _refused(lib.sa_flame_stats(x, 2, L.SA_F32, 16, P16, None, P8, 0, None), "required")
    _refused(lib.sa_flame_stats(x, 2, L.SA_F32, 16, P16, P8, None, 0, None), "required")
    _refused(lib.sa_flame_stats(x, 2, L.SA_F32, 0, P16, P8, None, 0, None), "required")  # stats even for n == 0
    _refused(lib.sa_flame_stats(_table(P16, 0), 2, L.SA_F32, 16, P16, P8, P8, 0, None), "client 1")
    _refused(lib.sa_flame_stats(_table(ODD, P16), 2, L.SA_F32, 16, P16, P8, P8, 0, None), "client 0")
    _refused(lib.sa_flame_stats(_table(P16, C.c_void_p(0x1004)), 2, L.SA_F64, 16, P16, P8, P8, 0, None), "aligned")
    _refused(lib.sa_flame_stats(x, 2, L.SA_F32, 16, ODD, P8, P8, 0, None), "aligned")
    _refused(lib.sa_flame_stats(x, 2, L.SA_F32, 16, P16, C.c_void_p(0x2004), P8, 0, None), "aligned")
    _refused(lib.sa_flame_stats(x, 2, L.SA_F32, 16, P16, P8, C.c_void_p(0x2004), 0, None), "aligned")
    _refused(lib.sa_flame_combine(None, s, w, 2, L.SA_F32, 16, P16, 2.0, P8, None), "required")
    _refused(lib.sa_flame_combine(x, None, w, 2, L.SA_F32, 16, P16, 2.0, P8, None), "required")
    _refused(lib.sa_flame_combine(x, s, None, 2, L.SA_F32, 16, P16, 2.0, P8, None), "required")
    _refused(lib.sa_flame_combine(x, s, w, 2, L.SA_F32, 16, None, 2.0, P8, None), "required")
    _refused(lib.sa_flame_combine(x, s, w, 2, L.SA_F32, 16, P16, 2.0, None, None), "required")
    _refused(lib.sa_flame_combine(_table(P16, 0), s, w, 2, L.SA_F32, 16, P16, 2.0, P8, None), "client 1")
    _refused(lib.sa_flame_combine(_table(P16, ODD), s, w, 2, L.SA_F32, 16, P16, 2.0, P8, None), "client 1")
    _refused(lib.sa_flame_combine(x, s, w, 2, L.SA_F32, 16, ODD, 2.0, P8, None), "aligned")
    _refused(lib.sa_flame_combine(x, s, w, 2, L.SA_F32, 16, P16, 2.0, C.c_void_p(0x2004), None), "aligned")
    # a NaN weight drops a client: every client dropped is refused, and a dropped client's pointer is not looked at
    nan = float("nan")
    _refused(lib.sa_flame_combine(x, s, _doubles(nan, nan), 2, L.SA_F32, 16, P16, 2.0, P8, None), "dropped")
    assert lib.sa_flame_combine(_table(P16, 0), s, _doubles(1.0, nan), 2, L.SA_F32, 0, None, 1.0, None, None) == L.SA_OK


def test_an_empty_combine_launches_nothing():
    lib = L.lib()
    assert lib.sa_flame_combine(_table(0, 0), _doubles(1.0, 1.0), _doubles(1.0, 1.0), 2, L.SA_F64, 0, None, 2.0, None,
                                None) == L.SA_OK


def test_the_wrappers_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    from sfl_amd import kernels as K

    x, out = torch.ones(8), torch.zeros(8, dtype=torch.float64)
    with pytest.raises(ValueError, match="device-resident"):
        K.flame_stats([x, x], torch.empty(8), torch.empty(64, dtype=torch.uint8), torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="device-resident"):
        K.flame_combine([x, x], [1.0, 1.0], [1.0, 1.0], [True, True], x, 2.0, out)
    with pytest.raises(TypeError):
        K.flame_scratch_bytes(16, 2, torch.int64)
    assert K.flame_scratch_bytes(16, 2, torch.float32) == 5 * 8 and K.flame_stat_count(16) == 152
