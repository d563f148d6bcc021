"""What the compression entries (sa_stc*, sa_scr*, sa_coo_*, sa_quant_*,
sa_dequant_*) refuse before any launch, without a GPU: for every class of
argument an entry checks, the return code and the full text of
sa_last_error().  The addresses below are never dereferenced: every call is
either refused or, with nothing to do, returns before a launch."""
from sfl_amd import _lib as L

F32, F64, I64 = L.SA_F32, L.SA_F64, L.SA_I64
# distinct 16-byte aligned addresses, one that is 2-byte aligned and one that is only byte-aligned
A, B, R, S, RES, ACC, MU, SCR = (0x1000 * k for k in range(1, 9))
P4, P8, ODD, BYTE = 0x1000, 0x2000, 0x1002, 0x1001
BAD_TYPES = (I64, 7, -1)

X_TYPE = "x_type must be SA_F32 or SA_F64"
ELEM_TYPE = "the element type must be SA_F32 or SA_F64"
N31 = "n must be below 2^31 (the flat index is int32)"
N32 = "n must be below 2^32"


def refused(rc, text):
    assert rc == L.SA_ERR_ARG, (rc, text)
    assert L.lib().sa_last_error().decode() == text


# ---------------------------------------------------------------------------
# sa_stc
# ---------------------------------------------------------------------------
STC_ARGS = ("sa_stc: bad arguments (a, sparse_out, res_out and scratch are required; element-aligned vectors, "
            "8-byte aligned scratch)")
STC_ALIAS = "sa_stc: only res_out may alias r"


def stc(a=A, b=B, r=R, xt=F32, n=64, m=8, sparse=S, res=RES, acc=ACC, mu=MU, scratch=SCR):
    return L.lib().sa_stc(a, b, r, xt, n, m, sparse, res, acc, mu, scratch, None)


def test_stc_scratch_bytes():
    lib = L.lib()
    for xt in BAD_TYPES:
        refused(lib.sa_stc_scratch_bytes(64, xt), "sa_stc_scratch_bytes: " + X_TYPE)
    for n in (2**32, 2**33, 2**64 - 1):
        refused(lib.sa_stc_scratch_bytes(n, F32), "sa_stc_scratch_bytes: " + N32)
    refused(lib.sa_stc_scratch_bytes(2**32, I64), "sa_stc_scratch_bytes: " + X_TYPE)  # the type is checked first
    for n, xt in ((0, F32), (1, F64), (2**32 - 1, F32)):
        rc = lib.sa_stc_scratch_bytes(n, xt)
        assert rc > 0 and rc % 8 == 0


def test_stc_type_size_and_mask_num():
    for xt in BAD_TYPES:
        refused(stc(xt=xt), "sa_stc: " + X_TYPE)
    for n in (2**32, 2**33):
        refused(stc(n=n, xt=F64), "sa_stc: n must be below 2^32 (ranks and counts are 32-bit)")
    refused(stc(n=64, m=65), "sa_stc: mask_num exceeds n")
    refused(stc(n=0, m=1), "sa_stc: mask_num exceeds n")
    refused(stc(xt=I64, n=2**32, m=2**33), "sa_stc: " + X_TYPE)  # type, then size, then mask_num
    refused(stc(n=2**32, m=2**33), "sa_stc: n must be below 2^32 (ranks and counts are 32-bit)")


def test_stc_required_pointers_and_alignment():
    for name in ("a", "sparse", "res", "scratch"):
        refused(stc(**{name: None}), STC_ARGS)
    for name in ("a", "b", "r", "sparse", "res", "acc", "mu"):
        refused(stc(**{name: BYTE}), STC_ARGS)
        refused(stc(**{name: ODD}), STC_ARGS)
        refused(stc(xt=F64, **{name: 0x1004}), STC_ARGS)  # float32-aligned is not float64-aligned
    refused(stc(scratch=SCR + 4), STC_ARGS)
    refused(stc(xt=F32, scratch=BYTE), STC_ARGS)


def test_stc_forbidden_aliasing():
    for kw in (dict(res=A), dict(res=B), dict(sparse=RES), dict(sparse=A), dict(sparse=B), dict(sparse=R),
               dict(acc=RES), dict(acc=S), dict(acc=A)):
        refused(stc(**kw), STC_ALIAS)
    refused(stc(b=None, r=None, acc=None, mu=None, sparse=A), STC_ALIAS)  # with the optional vectors absent


def test_stc_of_nothing_is_ok():
    assert stc(a=None, b=None, r=None, n=0, m=0, sparse=None, res=None, acc=None, mu=None, scratch=None) == L.SA_OK
    assert stc(a=BYTE, n=0, m=0, xt=F64) == L.SA_OK  # n == 0 returns before the pointers are looked at


# ---------------------------------------------------------------------------
# sa_scr
# ---------------------------------------------------------------------------
SCR_ARGS = ("sa_scr: bad arguments (a, sparse_out and scratch are required; element-aligned vectors, "
            "4-byte aligned stats_out, 8-byte aligned scratch)")
SCR_ALIAS = "sa_scr: only res_out may alias r"
SCR_ZERO = "rows, cols and inner must be positive"
SCR_BIG = "rows * cols * inner must be below 2^32 (indices and counts are 32-bit)"
SCR_2GIB = "the shape needs 2 GiB of scratch or more"
STATS = 0x9000


def scr(a=A, b=B, r=R, xt=F32, shape=(8, 8, 1), sparse=S, res=RES, stats=STATS, scratch=SCR):
    return L.lib().sa_scr(a, b, r, xt, *shape, 0.5, sparse, res, stats, scratch, None)


def both_scr(xt, shape, text):
    refused(L.lib().sa_scr_scratch_bytes(*shape, xt), "sa_scr_scratch_bytes: " + text)
    refused(scr(xt=xt, shape=shape), "sa_scr: " + text)


def test_scr_type_and_shape():
    for xt in BAD_TYPES:
        both_scr(xt, (8, 8, 1), X_TYPE)
    both_scr(I64, (0, 8, 1), X_TYPE)  # the type is checked first
    for shape in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (0, 0, 0), (0, 2**32, 1)):
        both_scr(F32, shape, SCR_ZERO)
    for shape in ((2**32, 1, 1), (1, 2**32, 1), (1, 1, 2**32), (1, 2**16, 2**16), (2**16, 2**16, 1),
                  (2**20, 2**10, 2**3), (2**31, 2**31, 4), (2**63, 2, 1)):
        both_scr(F64, shape, SCR_BIG)
    both_scr(F32, (2**29, 1, 1), SCR_2GIB)  # 2^29 row sums of 8 bytes
    lib = L.lib()
    for shape in ((8, 8, 1), (1, 1, 1), (3, 5, 7), (2**16, 2**15, 1)):
        rc = lib.sa_scr_scratch_bytes(*shape, F32)
        assert rc > 0 and rc % 8 == 0
        assert rc == lib.sa_scr_scratch_bytes(*shape, F64)  # a function of the shape only


def test_scr_required_pointers_and_alignment():
    for name in ("a", "sparse", "scratch"):
        refused(scr(**{name: None}), SCR_ARGS)
    for name in ("a", "b", "r", "sparse", "res"):
        refused(scr(**{name: BYTE}), SCR_ARGS)
        refused(scr(**{name: ODD}), SCR_ARGS)
        refused(scr(xt=F64, **{name: 0x1004}), SCR_ARGS)
    refused(scr(stats=STATS + 2), SCR_ARGS)
    refused(scr(stats=BYTE), SCR_ARGS)
    refused(scr(scratch=SCR + 4), SCR_ARGS)


def test_scr_forbidden_aliasing():
    for kw in (dict(sparse=A), dict(sparse=B), dict(sparse=R), dict(res=A), dict(res=B), dict(res=S)):
        refused(scr(**kw), SCR_ALIAS)
    refused(scr(b=None, r=None, res=None, stats=None, sparse=A), SCR_ALIAS)


# ---------------------------------------------------------------------------
# sa_coo_*
# ---------------------------------------------------------------------------
def coo_calls(xt=F32, n=16, at=F64):
    """name -> a call of every sa_coo entry that takes a type and a size, otherwise well-formed."""
    lib = L.lib()
    return {
        "sa_coo_scratch_bytes": lambda: lib.sa_coo_scratch_bytes(n, xt),
        "sa_coo_count": lambda: lib.sa_coo_count(P8, xt, n, P4, P4, None),
        "sa_coo_fill": lambda: lib.sa_coo_fill(P8, xt, n, P4, P4, P8, 0, P4, None),
        "sa_coo_decode": lambda: lib.sa_coo_decode(P4, P8, xt, 0, n, P8, P4, None),
        "sa_coo_axpy": lambda: lib.sa_coo_axpy(P4, P8, xt, 0, 1.0, P8, at, n, P4, None),
        "sa_coo_finish": lambda: lib.sa_coo_finish(P8, xt, n, 2.0, None),
    }


def test_coo_type_and_size():
    for xt in BAD_TYPES:
        for name, call in coo_calls(xt=xt).items():
            refused(call(), f"{name}: {ELEM_TYPE}")
    for n in (2**31, 2**32, 2**64 - 1):
        for name, call in coo_calls(n=n).items():
            refused(call(), f"{name}: {N31}")
    for name, call in coo_calls(xt=I64, n=2**31).items():
        refused(call(), f"{name}: {ELEM_TYPE}")  # the type is checked first
    for at in BAD_TYPES:
        refused(coo_calls(at=at)["sa_coo_axpy"](), "sa_coo_axpy: " + ELEM_TYPE)
        refused(coo_calls(at=at, n=2**31)["sa_coo_axpy"](), "sa_coo_axpy: " + ELEM_TYPE)
    lib = L.lib()
    for n, xt in ((0, F32), (16, F64), (2**31 - 1, F32)):
        rc = lib.sa_coo_scratch_bytes(n, xt)
        assert rc > 0 and rc % 4 == 0


def test_coo_count_pointers():
    lib = L.lib()
    text = ("sa_coo_count: bad arguments (x, scratch and nnz_out are required; element-aligned x, "
            "4-byte aligned scratch and nnz_out)")
    refused(lib.sa_coo_count(None, F32, 16, P4, P4, None), text)
    refused(lib.sa_coo_count(P4, F32, 16, None, P4, None), text)
    refused(lib.sa_coo_count(P4, F32, 16, P4, None, None), text)
    refused(lib.sa_coo_count(None, F32, 0, None, P4, None), text)  # scratch and nnz_out even for n == 0
    refused(lib.sa_coo_count(None, F32, 0, P4, None, None), text)
    refused(lib.sa_coo_count(BYTE, F32, 16, P4, P4, None), text)
    refused(lib.sa_coo_count(0x1004, F64, 16, P4, P4, None), text)
    refused(lib.sa_coo_count(P4, F32, 16, ODD, P4, None), text)
    refused(lib.sa_coo_count(P4, F32, 16, P4, BYTE, None), text)


def test_coo_fill_cap_and_pointers():
    lib = L.lib()
    refused(lib.sa_coo_fill(P8, F32, 16, P4, P4, P8, 17, P4, None), "sa_coo_fill: cap exceeds n")
    refused(lib.sa_coo_fill(None, F32, 0, P4, P4, P8, 1, P4, None), "sa_coo_fill: cap exceeds n")
    text = ("sa_coo_fill: bad arguments (x, scratch, flag and, for cap > 0, index_out and data_out are "
            "required; element-aligned vectors)")
    good = dict(x=P8, scratch=P4, index=0x3000, data=0x4000, cap=4, flag=0x5000)

    def fill(xt=F32, n=16, **kw):
        a = {**good, **kw}
        return lib.sa_coo_fill(a["x"], xt, n, a["scratch"], a["index"], a["data"], a["cap"], a["flag"], None)

    for name in ("x", "scratch", "index", "data", "flag"):
        refused(fill(**{name: None}), text)
        refused(fill(**{name: BYTE}), text)
    refused(fill(n=0, cap=0, x=None, scratch=None), text)  # scratch and flag even for n == 0
    refused(fill(n=0, cap=0, x=None, flag=None), text)
    refused(fill(xt=F64, x=0x1004), text)
    refused(fill(xt=F64, data=0x1004), text)
    refused(fill(cap=0, index=ODD, data=None), text)  # a pointer that is given is aligned, cap or no cap
    refused(fill(cap=0, index=None, data=BYTE), text)


def test_coo_payload_and_dense_pointers():
    lib = L.lib()
    for name, call in (
            ("sa_coo_decode", lambda i, d, xt, nnz, n, f: lib.sa_coo_decode(i, d, xt, nnz, n, P8, f, None)),
            ("sa_coo_axpy", lambda i, d, xt, nnz, n, f: lib.sa_coo_axpy(i, d, xt, nnz, 1.0, P8, F64, n, f, None))):
        refused(call(P4, P8, F32, 17, 16, P4), f"{name}: more entries than the tensor has elements")
        refused(call(P4, P8, F32, 1, 0, P4), f"{name}: more entries than the tensor has elements")
        text = f"{name}: bad arguments (index, data and flag are required; element-aligned vectors)"
        refused(call(None, P8, F32, 4, 16, P4), text)
        refused(call(P4, None, F32, 4, 16, P4), text)
        refused(call(P4, P8, F32, 4, 16, None), text)
        refused(call(None, None, F32, 0, 16, None), text)  # the flag record even for an empty payload
        refused(call(ODD, P8, F32, 4, 16, P4), text)
        refused(call(P4, BYTE, F32, 4, 16, P4), text)
        refused(call(P4, 0x1004, F64, 4, 16, P4), text)
        refused(call(P4, P8, F32, 4, 16, ODD), text)
        refused(call(None, None, F32, 0, 16, BYTE), text)
    text = "sa_coo_decode: dense_out is required and element-aligned"
    refused(lib.sa_coo_decode(P4, P8, F32, 4, 16, None, P4, None), text)
    refused(lib.sa_coo_decode(P4, P8, F32, 4, 16, BYTE, P4, None), text)
    refused(lib.sa_coo_decode(P4, P8, F64, 4, 16, 0x1004, P4, None), text)
    refused(lib.sa_coo_decode(None, None, F32, 0, 0, ODD, P4, None), text)
    for at, acc in ((F32, None), (F64, None), (F32, BYTE), (F64, 0x1004)):
        refused(lib.sa_coo_axpy(P4, P8, F32, 4, 1.0, acc, at, 16, P4, None),
                "sa_coo_axpy: acc is required and element-aligned")
    for acc in (None, BYTE, ODD):
        refused(lib.sa_coo_finish(acc, F32, 16, 2.0, None), "sa_coo_finish: acc is required and element-aligned")
    refused(lib.sa_coo_finish(0x1004, F64, 16, 2.0, None), "sa_coo_finish: acc is required and element-aligned")
    refused(lib.sa_coo_finish(BYTE, F32, 0, 2.0, None), "sa_coo_finish: acc is required and element-aligned")


def test_coo_axpy_refuses_float64_data_into_a_float32_accumulator():
    lib = L.lib()
    text = "sa_coo_axpy: float64 data needs a float64 accumulator"
    refused(lib.sa_coo_axpy(P4, P8, F64, 4, 1.0, P8, F32, 16, P4, None), text)
    refused(lib.sa_coo_axpy(None, None, F64, 0, 1.0, None, F32, 16, None, None), text)  # before the pointers
    refused(lib.sa_coo_axpy(P4, P8, F64, 17, 1.0, P8, F32, 16, P4, None), text)  # and before the payload's size
    refused(lib.sa_coo_axpy(P4, P8, F64, 4, 1.0, P8, F32, 2**31, P4, None), "sa_coo_axpy: " + N31)  # after the size


def test_coo_of_nothing_is_ok():
    lib = L.lib()
    assert lib.sa_coo_decode(None, None, F32, 0, 0, None, P4, None) == L.SA_OK
    assert lib.sa_coo_axpy(None, None, F32, 0, 1.0, None, F64, 0, P4, None) == L.SA_OK
    assert lib.sa_coo_axpy(None, None, F32, 0, 1.0, P8, F32, 16, P4, None) == L.SA_OK  # an empty payload
    assert lib.sa_coo_axpy(None, None, F64, 0, 1.0, P8, F64, 2**31 - 1, P4, None) == L.SA_OK
    assert lib.sa_coo_finish(None, F64, 0, 2.0, None) == L.SA_OK


# ---------------------------------------------------------------------------
# sa_quant_* / sa_dequant_*
# ---------------------------------------------------------------------------
def quant_calls(xt=F32, n=16, x=P8, q=P4, qb=1, mode=0, qmin=-128, qmax=127, fmt=(8, 6), scratch=P8, out3=0x3000):
    """name -> a call of every quantizer entry; ``x`` is the float vector, ``q`` the codes."""
    lib = L.lib()
    return {
        "sa_quant_scratch_bytes": lambda: lib.sa_quant_scratch_bytes(n, xt),
        "sa_quant_range": lambda: lib.sa_quant_range(x, xt, n, scratch, out3, None),
        "sa_quant_affine": lambda: lib.sa_quant_affine(x, xt, n, mode, 1.0, 0.0, qmin, qmax, q, qb, None),
        "sa_dequant_affine": lambda: lib.sa_dequant_affine(q, qb, n, mode, 1.0, 0.0, xt, x, None),
        "sa_quant_fp8": lambda: lib.sa_quant_fp8(x, xt, n, 1.0, *fmt, q, None),
        "sa_dequant_fp8": lambda: lib.sa_dequant_fp8(q, n, 1.0, *fmt, xt, x, None),
    }


CODED = ("sa_quant_affine", "sa_dequant_affine", "sa_quant_fp8", "sa_dequant_fp8")


def test_quant_type_and_size():
    for xt in BAD_TYPES:
        for name, call in quant_calls(xt=xt).items():
            refused(call(), f"{name}: {ELEM_TYPE}")
    for n in (2**32, 2**33, 2**64 - 1):
        for name, call in quant_calls(n=n).items():
            refused(call(), f"{name}: {N32}")
    for name, call in quant_calls(xt=I64, n=2**32, qb=3, mode=5, fmt=(0, 0), x=None).items():
        refused(call(), f"{name}: {ELEM_TYPE}")  # the type first, the size second, then everything else
    for name, call in quant_calls(n=2**32, qb=3, mode=5, fmt=(0, 0), x=None).items():
        refused(call(), f"{name}: {N32}")
    lib = L.lib()
    for n, xt in ((0, F64), (16, F32), (2**32 - 1, F32)):
        rc = lib.sa_quant_scratch_bytes(n, xt)
        assert rc > 0 and rc % 8 == 0


def test_quant_range_pointers():
    text = ("sa_quant_range: bad arguments (x, scratch and out3 are required; element-aligned x and out3, "
            "8-byte aligned scratch)")
    for kw in (dict(x=None), dict(scratch=None), dict(out3=None), dict(n=0, x=None, scratch=None),
               dict(n=0, x=None, out3=None), dict(x=BYTE), dict(x=ODD), dict(xt=F64, x=0x1004), dict(scratch=0x1004),
               dict(scratch=BYTE), dict(out3=BYTE), dict(xt=F64, out3=0x1004)):
        refused(quant_calls(**kw)["sa_quant_range"](), text)


def test_quant_vectors_code_width_mode_clamp_and_format():
    for name in CODED:
        text = f"{name}: bad arguments (the data and the codes are required; element-aligned vectors)"
        for kw in (dict(x=None), dict(q=None), dict(x=BYTE), dict(x=ODD), dict(xt=F64, x=0x1004),
                   dict(n=0, x=BYTE, q=None)):
            refused(quant_calls(**kw)[name](), text)
    for name in ("sa_quant_affine", "sa_dequant_affine"):
        for qb in (0, 3, 4, 8, -1):
            refused(quant_calls(qb=qb)[name](), f"{name}: q_bytes must be 1 (int8 codes) or 2 (int16 codes)")
        refused(quant_calls(qb=2, q=BYTE)[name](),
                f"{name}: bad arguments (the data and the codes are required; element-aligned vectors)")
        for mode in (-1, 2):
            refused(quant_calls(mode=mode)[name](), f"{name}: mode must be SA_QUANT_ZERO_POINT or SA_QUANT_LSTM")
    for qmin, qmax, qb in ((-129, 127, 1), (-128, 128, 1), (5, 5, 1), (7, -8, 1), (-32769, 0, 2), (0, 32768, 2)):
        refused(quant_calls(qmin=qmin, qmax=qmax, qb=qb)["sa_quant_affine"](),
                "sa_quant_affine: [qmin, qmax] must be a range inside the codes' storage type")
    for name in ("sa_quant_fp8", "sa_dequant_fp8"):
        for fmt in ((8, 14), (4, 6), (0, 0), (16, 6), (-8, 6)):
            refused(quant_calls(fmt=fmt)[name](),
                    f"{name}: (mant_len, exp_offset) must be (8, 6) for E4M3 or (4, 14) for E5M2")


def test_quant_of_nothing_is_ok():
    for xt in (F32, F64):
        for qb in (1, 2):
            calls = quant_calls(xt=xt, n=0, x=None, q=None, qb=qb, fmt=(4, 14) if qb == 2 else (8, 6))
            for name in CODED:
                assert calls[name]() == L.SA_OK, name
