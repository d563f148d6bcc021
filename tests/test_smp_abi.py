"""The sa_smp_* entries without a GPU: the library exports them, the header
declares what sfl_amd/_lib.py binds, and the arguments that can be refused
before any launch are refused, naming the argument."""
import ctypes as C
import os
import re

import pytest
from abi_header import ROOT, header

from sfl_amd import _lib as L

ENTRIES = ("sa_smp_mask_host", "sa_smp_mask", "sa_smp_delta_f32", "sa_smp_sumsq_f32", "sa_smp_perturb_f32",
           "sa_smp_finish_f32")
# addresses that are never dereferenced: every call below is refused before any launch
P16, Q16, R16, P8, ODD = (C.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x2008, 0x1004))


def _kinds():
    """The prototypes' parameter types as the binding states them.  Looked up when a test runs:
    tests/test_boundary.py reloads sfl_amd._lib, which makes its structure classes anew."""
    return {"float*": C.c_void_p, "double*": C.c_void_p, "uint8_t*": C.c_void_p, "void*": C.c_void_p,
            "uint64_t": C.c_uint64, "int": C.c_int, "sa_smp*": C.POINTER(L.SMP), "sa_dp*": C.POINTER(L.DP)}


def _smp(counter0=0, threshold=2**31, divisor=0.5, key=1):
    return L.SMP(key, counter0, threshold, divisor)


def _dp(counter0=0, sumsq=0x4000, num_updates=2.0):
    return L.DP(sumsq, None, 1.0, 0.0, num_updates, 7, counter0)


def _refused(rc, *words):
    assert rc == L.SA_ERR_ARG
    for w in words:
        assert w.encode() in L.lib().sa_last_error(), L.lib().sa_last_error()


def test_the_library_exports_the_entries():
    lib = L.lib()
    for name in ENTRIES:
        assert name in L.EXPORTED, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.sa_abi_version() == 3 and L.ABI_VERSION == 3  # the entries are additive


def test_the_header_declares_what_the_binding_binds():
    want = {
        "sa_smp_mask_host": "int sa_smp_mask_host(const sa_smp* smp, uint64_t n, uint8_t* out);",
        "sa_smp_mask": "int sa_smp_mask(const sa_smp* smp, uint64_t n, uint8_t* out, void* stream);",
        "sa_smp_delta_f32": "int sa_smp_delta_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, "
                            "float* out, void* stream);",
        "sa_smp_sumsq_f32": "int sa_smp_sumsq_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, "
                            "double* partials, double* sumsq, int accumulate, void* stream);",
        "sa_smp_perturb_f32": "int sa_smp_perturb_f32(const float* w0, const float* w1, uint64_t n, const sa_smp* smp, "
                              "const sa_dp* dp, float* out, void* stream);",
        "sa_smp_finish_f32": "int sa_smp_finish_f32(const float* w0, const float* t, uint64_t n, const sa_smp* smp, "
                             "float* out, void* stream);",
    }
    assert set(want) == set(ENTRIES)
    hdr = header()
    flat = " ".join(hdr.split())
    lib, kinds = L.lib(), _kinds()
    for name, proto in want.items():
        assert proto in flat, name
        types = [kinds[p.replace("const ", "", 1).rsplit(" ", 1)[0]]
                 for p in proto[proto.index("(") + 1:proto.rindex(")")].split(", ")]
        assert list(getattr(lib, name).argtypes) == types, name
    assert re.search(r"#define SA_ABI_VERSION 3\b", hdr)
    assert re.search(r"typedef struct sa_smp \{\s*uint64_t key;[^}]*uint64_t counter0;[^}]*uint64_t threshold;"
                     r"[^}]*float divisor;[^}]*\} sa_smp;", hdr)
    assert C.sizeof(L.SMP) == 32 and [f[0] for f in L.SMP._fields_] == ["key", "counter0", "threshold", "divisor"]
    assert (L.SMP.key.offset, L.SMP.counter0.offset, L.SMP.threshold.offset, L.SMP.divisor.offset) == (0, 8, 16, 24)


def test_the_header_carries_the_definition():
    hdr = open(os.path.join(ROOT, "include", "sfl_sa.h")).read()
    for phrase in ("FedSMP_torch.py:105-119", "w_i < threshold", "hi32(i >> 2), 1, 0)", "kept ? w0 + t : w0",
                   "np.float32(p + 1e-6)"):
        assert phrase in hdr, phrase


def _calls(lib, smp, w0=P16, w1=Q16, out=R16, part=P8, sumsq=P8, n=16, dp=None):
    """Every device entry with the given arguments: (name, return code)."""
    s = C.byref(smp) if smp is not None else None
    d = C.byref(dp) if dp is not None else None
    return {"sa_smp_delta_f32": lambda: lib.sa_smp_delta_f32(w0, w1, n, s, out, None),
            "sa_smp_finish_f32": lambda: lib.sa_smp_finish_f32(w0, w1, n, s, out, None),
            "sa_smp_sumsq_f32": lambda: lib.sa_smp_sumsq_f32(w0, w1, n, s, part, sumsq, 0, None),
            "sa_smp_perturb_f32": lambda: lib.sa_smp_perturb_f32(w0, w1, n, s, d, out, None),
            "sa_smp_perturb_f32/dp": lambda: lib.sa_smp_perturb_f32(w0, w1, n, s, C.byref(dp if dp is not None else _dp()),
                                                                    out, None)}


def test_a_bad_mask_is_refused_before_any_launch():
    lib = L.lib()
    out = (C.c_uint8 * 16)()
    for bad, word in ((_smp(counter0=2), "counter0"), (_smp(counter0=4097), "counter0"),
                      (_smp(threshold=2**32 + 1), "threshold"), (_smp(threshold=2**63), "threshold")):
        _refused(lib.sa_smp_mask_host(C.byref(bad), 16, out), "sa_smp_mask_host", word)
        _refused(lib.sa_smp_mask(C.byref(bad), 16, P16, None), "sa_smp_mask", word)
        for name, call in _calls(lib, bad).items():
            _refused(call(), name.split("/")[0], word)
        for name, call in _calls(lib, bad, n=0).items():  # the mask is looked at even for n == 0
            _refused(call(), word)
    _refused(lib.sa_smp_mask_host(None, 16, out), "smp is required")
    for name, call in _calls(lib, None).items():
        _refused(call(), name.split("/")[0], "smp is required")
    # the entries that divide want a positive divisor; the others do not look at it
    for div in (0.0, -1.0, float("nan")):
        bad = _smp(divisor=div)
        for name, call in _calls(lib, bad).items():
            if name == "sa_smp_finish_f32":
                continue
            _refused(call(), name.split("/")[0], "divisor")
        assert lib.sa_smp_mask_host(C.byref(bad), 16, out) == L.SA_OK
    assert lib.sa_smp_mask_host(C.byref(_smp(threshold=2**32)), 16, out) == L.SA_OK and all(out)
    assert lib.sa_smp_mask_host(C.byref(_smp(threshold=0)), 16, out) == L.SA_OK and not any(out)


def test_null_and_misaligned_pointers_are_refused_naming_the_argument():
    lib = L.lib()
    smp = _smp()
    for name, call in _calls(lib, smp, w0=None).items():
        _refused(call(), name.split("/")[0], "w0 is required")
    for name, call in _calls(lib, smp, w0=ODD).items():
        _refused(call(), name.split("/")[0], "w0 must be 16-byte aligned")
    second = {"sa_smp_finish_f32": "t"}
    for name, call in _calls(lib, smp, w1=None).items():
        _refused(call(), f"{second.get(name, 'w1')} is required")
    for name, call in _calls(lib, smp, w1=P8).items():
        _refused(call(), f"{second.get(name, 'w1')} must be 16-byte aligned")
    for name, call in _calls(lib, smp, out=None).items():
        if name != "sa_smp_sumsq_f32":
            _refused(call(), "out is required")
    for name, call in _calls(lib, smp, out=ODD).items():
        if name != "sa_smp_sumsq_f32":
            _refused(call(), "out must be 16-byte aligned")
    _refused(lib.sa_smp_sumsq_f32(P16, Q16, 16, C.byref(smp), None, P8, 0, None), "partials is required")
    _refused(lib.sa_smp_sumsq_f32(P16, Q16, 16, C.byref(smp), P8, None, 0, None), "sumsq is required")
    _refused(lib.sa_smp_sumsq_f32(P16, Q16, 0, C.byref(smp), P8, None, 0, None), "sumsq is required")  # even for n == 0
    _refused(lib.sa_smp_mask(C.byref(smp), 16, None, None), "out is required")
    _refused(lib.sa_smp_mask_host(C.byref(smp), 16, None), "out is required")


def test_a_bad_dp_is_refused():
    lib = L.lib()
    smp = C.byref(_smp())
    for bad in (_dp(counter0=6), _dp(sumsq=None), _dp(num_updates=0.0)):
        for n in (16, 0):
            _refused(lib.sa_smp_perturb_f32(P16, Q16, n, smp, C.byref(bad), R16, None), "sa_smp_perturb_f32", "sa_dp",
                     "counter0")


def test_an_n_beyond_the_tile_grid_is_refused():
    lib = L.lib()
    smp = _smp()
    for n in (2**41, 2**64 - 1):
        for name, call in _calls(lib, smp, n=n).items():
            _refused(call(), name.split("/")[0], "too large")
        _refused(lib.sa_smp_mask(C.byref(smp), n, P16, None), "too large")


def test_empty_calls_look_at_no_vector():
    lib = L.lib()
    smp = C.byref(_smp())
    assert lib.sa_smp_mask_host(smp, 0, None) == L.SA_OK
    assert lib.sa_smp_mask(smp, 0, None, None) == L.SA_OK
    assert lib.sa_smp_delta_f32(None, None, 0, smp, None, None) == L.SA_OK
    assert lib.sa_smp_finish_f32(ODD, ODD, 0, smp, ODD, None) == L.SA_OK
    assert lib.sa_smp_perturb_f32(None, None, 0, smp, None, None, None) == L.SA_OK
    assert lib.sa_smp_perturb_f32(None, None, 0, smp, C.byref(_dp()), None, None) == L.SA_OK


def test_the_wrappers_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    from sfl_amd import kernels as K

    x, smp = torch.ones(8), K.make_smp(1, 0, 2**31, 0.5)
    f64 = torch.zeros(1, dtype=torch.float64)
    for call in (lambda: K.smp_mask(smp, torch.zeros(8, dtype=torch.uint8)), lambda: K.smp_delta(x, x, smp, x),
                 lambda: K.smp_sumsq(x, x, smp, f64, torch.zeros(L.SA_DP_PARTIALS, dtype=torch.float64)),
                 lambda: K.smp_perturb(x, x, smp, None, x), lambda: K.smp_finish(x, x, smp, x)):
        with pytest.raises(ValueError, match="device-resident"):
            call()
    with pytest.raises(ValueError, match="multiple of 4"):
        K.make_smp(1, 2, 2**31, 0.5)
