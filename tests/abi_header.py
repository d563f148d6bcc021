"""include/sfl_sa.h against sfl_amd/_lib.py, for the ABI tests of the
compression entries (test_coo_abi.py, test_quant_abi.py, test_stc_scr_abi.py):
the header declares each entry with the prototype the test states, and the
binding's ``argtypes`` are that prototype's types."""
import ctypes as C
import os
import re

from sfl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"void*": C.c_void_p, "uint64_t": C.c_uint64, "int": C.c_int, "double": C.c_double}


def header():
    """The header's text without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfl_sa.h")).read(), flags=re.S)


def check_entries(want, macros=(), macro_suffix=""):
    """``want``: entry -> its prototype as one line; ``macros``: (name, value)
    pairs the header must ``#define`` (``macro_suffix``: e.g. ``u``)."""
    hdr = header()
    flat = " ".join(hdr.split())
    lib = L.lib()
    for name, proto in want.items():
        assert proto in flat, name
        params = proto[proto.index("(") + 1:proto.rindex(")")].split(", ")
        types = [KINDS[p.replace("const ", "").rsplit(" ", 1)[0]] for p in params]
        assert list(getattr(lib, name).argtypes) == types, name
    for macro, value in macros:
        assert re.search(r"#define %s %d%s\b" % (macro, value, macro_suffix), hdr), macro
    assert re.search(r"#define SA_ABI_VERSION 3\b", hdr)
