"""What the top-k entries (sa_topk_*, sa_coo_gather) refuse before any launch,
without a GPU: for every class of argument an entry checks, the return code
and the full text of sa_last_error(); that the library exports them and the
header declares what sfl_amd/_lib.py binds.  The addresses below are never
dereferenced: every call is either refused or, with nothing to do, returns
before a launch."""
import numpy as np
import pytest
from abi_header import check_entries

from sfl_amd import _lib as L

ENTRIES = ("sa_topk_scratch_bytes", "sa_topk_select", "sa_topk_fill", "sa_topk_random_keys",
           "sa_topk_random_keys_host", "sa_coo_gather")
F32, F64, I64 = L.SA_F32, L.SA_F64, L.SA_I64
# distinct 16-byte aligned addresses far apart, one that is 2-byte aligned and one that is only byte-aligned
KEYS, X, SCR, IDX, DATA, FLAG = (0x100000 * k for k in range(1, 7))
ODD, BYTE = 0x100002, 0x100001
BAD_TYPES = (I64, 7, -1)

KEY_TYPE = "key_type must be SA_F32 or SA_F64"
N31 = "n must be below 2^31 (the flat index is int32)"


def refused(rc, text):
    assert rc == L.SA_ERR_ARG, (rc, text)
    assert L.lib().sa_last_error().decode() == text


def select(keys=KEYS, kt=F32, n=64, k=8, scratch=SCR):
    return L.lib().sa_topk_select(keys, kt, n, k, scratch, None)


def fill(keys=KEYS, kt=F32, x=X, xt=F32, n=64, k=8, scratch=SCR, index=IDX, data=DATA, flag=FLAG):
    return L.lib().sa_topk_fill(keys, kt, x, xt, n, k, scratch, index, data, flag, None)


def gather(index=IDX, nnz=8, x=X, xt=F32, n=64, data=DATA, flag=FLAG):
    return L.lib().sa_coo_gather(index, nnz, x, xt, n, data, flag, None)


def test_the_library_exports_the_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.sa_abi_version() == 3  # the entries are additive


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_topk_scratch_bytes": "int sa_topk_scratch_bytes(uint64_t n, int key_type);",
        "sa_topk_select": "int sa_topk_select(const void* keys, int key_type, uint64_t n, uint64_t k, void* scratch, "
                          "void* stream);",
        "sa_topk_fill": "int sa_topk_fill(const void* keys, int key_type, const void* x, int x_type, uint64_t n, "
                        "uint64_t k, const void* scratch, void* index_out, void* data_out, void* flag, void* stream);",
        "sa_topk_random_keys": "int sa_topk_random_keys(uint64_t seed, uint64_t n, void* keys_out, void* stream);",
        "sa_topk_random_keys_host": "int sa_topk_random_keys_host(uint64_t seed, uint64_t n, void* keys_out);",
        "sa_coo_gather": "int sa_coo_gather(const void* index, uint64_t nnz, const void* x, int x_type, uint64_t n, "
                         "void* data_out, void* flag, void* stream);",
    }
    assert set(want) == set(ENTRIES)
    check_entries(want)


def test_scratch_bytes():
    lib = L.lib()
    for kt in BAD_TYPES:
        refused(lib.sa_topk_scratch_bytes(64, kt), "sa_topk_scratch_bytes: " + KEY_TYPE)
    for n in (2**31, 2**32, 2**64 - 1):
        refused(lib.sa_topk_scratch_bytes(n, F32), "sa_topk_scratch_bytes: " + N31)
    refused(lib.sa_topk_scratch_bytes(2**31, I64), "sa_topk_scratch_bytes: " + KEY_TYPE)  # the type is checked first
    sizes = {lib.sa_topk_scratch_bytes(n, kt) for n, kt in ((0, F32), (1, F64), (2**31 - 1, F32), (2**20, F64))}
    assert len(sizes) == 1  # a function of nothing but the layout's constants
    rc = sizes.pop()
    assert rc > 0 and rc % 8 == 0


def test_select_type_size_and_k():
    for kt in BAD_TYPES:
        refused(select(kt=kt), "sa_topk_select: " + KEY_TYPE)
    for n in (2**31, 2**33):
        refused(select(n=n, kt=F64), "sa_topk_select: " + N31)
    refused(select(n=64, k=65), "sa_topk_select: k exceeds n")
    refused(select(n=0, k=1), "sa_topk_select: k exceeds n")
    refused(select(kt=I64, n=2**31, k=2**33), "sa_topk_select: " + KEY_TYPE)  # type, then size, then k
    refused(select(n=2**31, k=2**33), "sa_topk_select: " + N31)


def test_select_pointers():
    text = ("sa_topk_select: bad arguments (keys and scratch are required; element-aligned keys, 8-byte aligned "
            "scratch)")
    for kw in (dict(keys=None), dict(scratch=None), dict(keys=BYTE), dict(keys=ODD), dict(kt=F64, keys=KEYS + 4),
               dict(scratch=SCR + 4), dict(scratch=BYTE), dict(k=0, keys=None), dict(k=64, scratch=None)):
        refused(select(**kw), text)


def test_fill_type_size_and_k():
    for t in BAD_TYPES:
        refused(fill(kt=t), "sa_topk_fill: " + KEY_TYPE)
        refused(fill(xt=t), "sa_topk_fill: x_type must be SA_F32 or SA_F64")
    refused(fill(kt=I64, xt=I64), "sa_topk_fill: " + KEY_TYPE)  # keys' type first
    for n in (2**31, 2**33):
        refused(fill(n=n), "sa_topk_fill: " + N31)
    refused(fill(xt=7, n=2**31, k=2**33), "sa_topk_fill: x_type must be SA_F32 or SA_F64")  # types, size, then k
    refused(fill(n=64, k=65), "sa_topk_fill: k exceeds n")
    refused(fill(n=0, k=1), "sa_topk_fill: k exceeds n")


def test_fill_pointers_and_aliasing():
    text = ("sa_topk_fill: bad arguments (keys, x, scratch, flag and, for k > 0, index_out and data_out are "
            "required; element-aligned vectors, 8-byte aligned scratch)")
    for name in ("keys", "x", "scratch", "index", "data", "flag"):
        refused(fill(**{name: None}), text)
        refused(fill(**{name: BYTE}), text)
    for kw in (dict(kt=F64, keys=KEYS + 4), dict(xt=F64, x=X + 4), dict(xt=F64, data=DATA + 4), dict(scratch=SCR + 4),
               dict(index=ODD), dict(flag=ODD), dict(k=0, index=ODD, data=None), dict(k=0, index=None, data=BYTE),
               dict(k=0, flag=None)):
        refused(fill(**kw), text)
    refused(fill(x=KEYS, xt=F64), "sa_topk_fill: x is keys itself only with keys' element type")
    alias = "sa_topk_fill: index_out and data_out may alias nothing"
    for kw in (dict(index=KEYS), dict(index=X), dict(data=KEYS), dict(data=X), dict(x=KEYS, data=KEYS),
               dict(index=DATA), dict(index=DATA + 16), dict(data=IDX + 28), dict(index=SCR), dict(data=SCR + 64),
               dict(index=FLAG), dict(data=FLAG + 4), dict(index=KEYS + 252), dict(data=X + 252),
               dict(index=X - 28), dict(kt=F64, data=KEYS + 508)):
        refused(fill(**kw), alias)


def test_random_keys():
    lib = L.lib()
    out = np.zeros(4, dtype=np.uint64)
    for name, call in (("sa_topk_random_keys", lambda n, p: lib.sa_topk_random_keys(1, n, p, None)),
                       ("sa_topk_random_keys_host", lambda n, p: lib.sa_topk_random_keys_host(1, n, p))):
        for n in (2**31, 2**40):
            refused(call(n, out.ctypes.data), f"{name}: {N31}")
        for p in (None, BYTE, ODD, KEYS + 4):
            refused(call(4, p), f"{name}: keys_out is required and 8-byte aligned")
    assert not out.any()
    assert lib.sa_topk_random_keys_host(1, 3, out.ctypes.data) == L.SA_OK
    assert out[:3].all() and out[3] == 0  # n words, not one more


def test_gather():
    for xt in BAD_TYPES:
        refused(gather(xt=xt), "sa_coo_gather: the element type must be SA_F32 or SA_F64")
    for n in (2**31, 2**32):
        refused(gather(n=n), "sa_coo_gather: " + N31)
    refused(gather(nnz=65), "sa_coo_gather: more entries than the tensor has elements")
    refused(gather(nnz=1, n=0), "sa_coo_gather: more entries than the tensor has elements")
    text = ("sa_coo_gather: bad arguments (flag and, for nnz > 0, index, x and data_out are required; "
            "element-aligned vectors)")
    for kw in (dict(index=None), dict(x=None), dict(data=None), dict(flag=None), dict(nnz=0, flag=None),
               dict(index=ODD), dict(x=BYTE), dict(data=BYTE), dict(flag=ODD), dict(xt=F64, x=X + 4),
               dict(xt=F64, data=DATA + 4), dict(nnz=0, index=ODD)):
        refused(gather(**kw), text)
    for kw in (dict(data=X), dict(data=X + 252), dict(data=IDX), dict(data=IDX + 28), dict(data=FLAG),
               dict(data=X - 28)):
        refused(gather(**kw), "sa_coo_gather: data_out may alias nothing")


def test_of_nothing_is_ok():
    lib = L.lib()
    assert select(keys=None, n=0, k=0, scratch=None) == L.SA_OK
    assert select(keys=BYTE, kt=F64, n=0, k=0) == L.SA_OK  # n == 0 returns before the pointers are looked at
    assert fill(keys=None, x=None, n=0, k=0, scratch=None, index=None, data=None, flag=None) == L.SA_OK
    assert fill(keys=BYTE, x=ODD, n=0, k=0, flag=BYTE) == L.SA_OK
    assert lib.sa_topk_random_keys(1, 0, None, None) == L.SA_OK
    assert lib.sa_topk_random_keys_host(1, 0, None) == L.SA_OK
    assert gather(index=None, nnz=0, x=None, n=0, data=None) == L.SA_OK  # the flag record even for nothing
    assert gather(index=None, nnz=0, data=None) == L.SA_OK


def test_the_wrappers_refuse_host_tensors_and_other_types():
    torch = pytest.importorskip("torch")
    from sfl_amd import kernels as K

    x = torch.ones(8)
    words = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="device-resident"):
        K.topk_select(x, 2, words)
    with pytest.raises(ValueError, match="device-resident"):
        K.topk_fill(x, x, 2, words, words, x[:2], words)
    with pytest.raises(ValueError, match="device-resident"):
        K.topk_random_keys(1, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="device-resident"):
        K.coo_gather(words, x, x[:2], words)
    with pytest.raises(TypeError):
        K.topk_scratch_bytes(16, torch.int64)
    assert K.topk_scratch_bytes(16, torch.float32) == K.topk_scratch_bytes(2**20, torch.float64)
