"""sa_scr on the GPU against the numpy restatement (tests/scr_oracle.py):
sparse and res bit for bit, the counts in stats_out.  On random data the
device is compared away from the thresholds only: the fixture's cases and the
operand forms keep every ratio at least 1e-5 / 1e-9 away (asserted on the CPU
by test_scr_oracle.py and in _form_case), because the device adds its float64
sums in another order than numpy, which moves a ratio by about 1e-13.  The
sums themselves are pinned at margin 0 by the decisive-element cases of
test_scr_oracle.py (DECISIVE): multiples of 2^-20 whose sums are exact in
every order, every structure at its threshold or one element away from it, at
the shapes that reach each launch geometry; and by
exact ties of small integers."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import scr_oracle as so  # noqa: E402
from gpu_copies import DEV, _bits, _dev, _host  # noqa: E402
from test_scr_oracle import DECISIVE, DECISIVE_IDS, THR, TIES, decisive, specials  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = ["f32", "f64"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scr_reference.npz")
# Beside the fixture's shapes, for the operand forms: float32 rows that are a
# multiple of 16 bytes and longer than a wave's segment (2048), so the
# 16-byte path meets a ragged last segment; an inner size above 1 on the
# 16-byte path; a row length just past one segment on the element path.
# Then the launch geometries of DESIGN.md section 13 that those leave out:
# two segments with more than 256 rows; three tiles with two rows per slab;
# conv rows longer than a segment on the 16-byte and on the element path;
# conv rows with two rows per slab.
FORM_SHAPES = ((64, 64), (65, 257), (1000, 3), (3, 100003), (65, 33, 3, 3), (5, 4100), (9, 4, 8, 8), (7, 2049),
               (300, 2049), (1100, 2052), (6, 260, 3, 3), (5, 229, 3, 3), (2100, 12, 3, 3))
# the sums differ from numpy's by at most n * 2^-53 relative (n <= 300009 here: 3.4e-11)
FORM_MARGIN = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def run(a, b=None, r=None, thr=0.0, want_res=True, alias=False, misalign=False, fill=None, stats=True):
    """(sparse, res, stats) as host arrays (res None without want_res)."""
    from sfl_amd import kernels as K

    v3 = so.view3(a.shape)
    ta, tb, tr = (_dev(x, misalign) for x in (a, b, r))
    sparse = _dev(np.full(a.shape, 7, a.dtype), misalign)
    res = None if not want_res else (tr if alias else _dev(np.full(a.shape, 7, a.dtype), misalign))
    st = torch.full((2,), 12345, dtype=torch.int32, device=DEV) if stats else None
    scratch = torch.empty(K.scr_scratch_bytes(v3, ta.dtype), dtype=torch.uint8, device=DEV)
    if fill is not None:
        scratch.fill_(fill)
    K.scr(ta, tb, tr, v3, thr, sparse, res, stats_out=st, scratch=scratch)
    torch.cuda.synchronize()
    return (_host(sparse).reshape(a.shape), None if res is None else _host(res).reshape(a.shape),
            None if st is None else _host(st))


def check(out, want, key=""):
    sparse, res, st = out
    w_sparse, w_res, rows, cols = want
    assert np.array_equal(_bits(sparse), _bits(w_sparse)), key
    if res is not None:
        assert np.array_equal(_bits(res), _bits(w_res)), key
    if st is not None:
        assert st.tolist() == [int(rows.sum()), int(cols.sum())], key


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", so.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fixture_cases_bit_for_bit(golden, dt, shape):
    u = None
    for thr in so.THRESHOLDS:
        key = so.case_key(dt, shape, thr)
        seed = int(golden[key + "_seed"])
        if u is None or seed != u[0]:
            u = (seed, so.case_input(seed, shape, dt))
        want = so.scr(u[1], thr=thr)
        check(run(u[1], thr=thr), want, key)
        check(run(u[1], thr=thr, want_res=False), want, key)


_forms = {}


def _form_case(dt, shape):
    """(a, b, r) and, per operand form and threshold, the restatement's
    result; computed once.  The margin of every formed update is asserted."""
    if (dt, shape) not in _forms:
        a, b, r = (so.case_input(s, shape, dt) for s in (11, 12, 13))
        r = (r * dt(0.25)).astype(dt)
        want = {}
        for name, (bb, rr) in {"ab": (b, None), "abr": (b, r), "a": (None, None)}.items():
            for thr in (0.3, 0.8):
                uu = so.form(a, bb, rr)
                _, _, r0, r1 = so.drop_flags(uu, thr)
                assert so.margin(r0, r1, thr) >= FORM_MARGIN, (shape, name, thr)
                want[name, thr] = so.scr(a, bb, rr, thr)
        _forms[dt, shape] = (a, b, r, want)
    return _forms[dt, shape]


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", FORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_operand_forms_alias_and_alignment(dt, shape):
    """Worker first round (a, b), worker with error feedback (a, b, r), after
    a DP pre-step (a); without res_out; res_out aliasing r; every vector
    offset by one element (element accesses, the same lane-to-element map)."""
    a, b, r, want = _form_case(dt, shape)
    for thr in (0.3, 0.8):
        for name, (bb, rr) in {"ab": (b, None), "abr": (b, r), "a": (None, None)}.items():
            w = want[name, thr]
            check(run(a, bb, rr, thr), w, (name, thr))
            check(run(a, bb, rr, thr, want_res=False), w, (name, thr))
            check(run(a, bb, rr, thr, misalign=True), w, (name, thr, "offset"))
            check(run(a, bb, rr, thr, want_res=False, misalign=True, stats=False), w, (name, thr, "offset"))
        check(run(a, b, r, thr, alias=True), want["abr", thr], "alias")
        check(run(a, None, r, thr, alias=True), so.scr(a, None, r, thr), "alias")


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
def test_ties_and_special_values(dt):
    for make in TIES:
        u, thr, rows_want, cols_want, want = make(dt)
        sparse, res, st = run(u, thr=thr)
        assert np.array_equal(_bits(sparse), _bits(want)), make.__name__
        assert st.tolist() == [sum(rows_want), sum(cols_want)], make.__name__
        check((sparse, res, st), so.scr(u, thr=thr), make.__name__)
    for name, u, thr, want in specials(dt):
        out = run(u, thr=thr)
        assert np.array_equal(_bits(out[0]), _bits(want)), name
        check(out, so.scr(u, thr=thr), name)
        check(run(u, thr=thr, want_res=False), so.scr(u, thr=thr), name)
    # the same ties with rows longer than a wave's segment and rows narrower than a wave
    for shape in ((3, 4100), (300, 4)):
        u = np.zeros(shape, dt)
        u[0, :4], u[1, -2:], u[2, 1] = [2, -1, 1, 0], [1, -1], 1
        sparse, res, st = run(u, thr=0.5)
        check((sparse, res, st), so.scr(u, thr=0.5), shape)
        assert sparse[0, 0] == 2 and np.count_nonzero(sparse) == 1 and st[0] == shape[0] - 1


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
@pytest.mark.parametrize("kind,shape", list(DECISIVE), ids=DECISIVE_IDS)
def test_decisive_elements_at_margin_zero(dt, kind, shape):
    """Every structure at its threshold, the sums exact in every order: a
    sum that loses or gains an element, or a bit, drops other structures
    than the restatement.  The case keeps its decisive structure, the twin
    drops it; dropped rows hold 2q in the columns at the tie, which go."""
    v3 = so.view3(shape)
    for where in DECISIVE[kind, shape]:
        u, twin, axis, j, gone, ties = decisive(kind, shape, where, dt)
        want, want_twin = so.scr(u, thr=THR), so.scr(twin, thr=THR)
        assert not want[2 + axis][j] and want_twin[2 + axis][j], where
        out = run(u, thr=THR)
        check(out, want, where)
        assert not out[0].reshape(v3)[:, ties].any() and not out[0].reshape(v3)[list(gone)].any(), where
        check(run(u, thr=THR, want_res=False), want, where)
        check(run(u, thr=THR, misalign=True), want, (where, "offset"))
        check(run(twin, thr=THR), want_twin, (where, "twin"))
        check(run(twin, thr=THR, want_res=False), want_twin, (where, "twin"))


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
def test_same_bits_on_every_run_and_whatever_the_scratch_held(dt):
    for shape in ((3, 100003), (4099, 33), (65, 33, 3, 3), (1100, 2052), (6, 260, 3, 3)):
        a, b, r = (so.case_input(s, shape, dt) for s in (11, 12, 13))
        one, two, three = run(a, b, r, 0.3), run(a, b, r, 0.3), run(a, b, r, 0.3, fill=0xFF)
        for x, y, z in zip(one, two, three):
            assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z)), shape


def test_compressor_takes_the_device_path():
    from sfl_amd.utils import compressor as Cz

    for shape in ((65, 257), (65, 33, 3, 3)):
        a, b, r, want = _form_case(np.float32, shape)
        ta, tb, tr = (_dev(x).view(a.shape) for x in (a, b, r))
        sparse, res = Cz.scr_step(ta, tb, tr, 0.3)
        assert sparse.is_cuda and res.is_cuda and sparse.shape == a.shape
        check((_host(sparse), _host(res), None), want["abr", 0.3])
        sparse, res = Cz.scr_step(ta, tb, None, 0.8, want_res=False)
        assert res is None
        check((_host(sparse), None, None), want["ab", 0.8])
    a, _, _, _ = _form_case(np.float32, (65, 257))
    t = _dev(np.ascontiguousarray(a.T)).view(a.shape[::-1]).t()  # not contiguous
    (sparse,) = Cz.SCRSparse(0.3)([t])
    check((_host(sparse), None, None), so.scr(a, thr=0.3))
    bias = torch.arange(5, dtype=torch.float32, device=DEV)
    sparse, res = Cz.scr_step(bias, None, None, 2.0)
    assert torch.equal(sparse, bias) and sparse.data_ptr() != bias.data_ptr() and not res.any()
    ints = _dev(np.array([[4, -2, 2], [1, 0, 0], [4, 2, 0]])).reshape(3, 3)
    sparse, res = Cz.scr_step(ints, None, None, 0.3)
    assert sparse.is_cuda and sparse.dtype == torch.int64
    assert _host(sparse).tolist() == [[4, -2, 0], [0, 0, 0], [4, 2, 0]] and torch.equal(sparse + res, ints)


def test_refusals_launch_nothing():
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    lib = L.lib()
    t = torch.full((192,), 3.0, dtype=torch.float32, device=DEV)
    s = torch.empty(K.scr_scratch_bytes((8, 8, 1), torch.float32), dtype=torch.uint8, device=DEV)
    p, sp = t.data_ptr(), s.data_ptr()
    before = t.clone()
    for xt, shp in ((L.SA_I64, (8, 8, 1)), (7, (8, 8, 1)), (L.SA_F32, (0, 8, 1)), (L.SA_F32, (8, 0, 1)),
                    (L.SA_F64, (8, 8, 0)), (L.SA_F32, (2**16, 2**16, 1)), (L.SA_F64, (2**20, 2**10, 2**3))):
        assert lib.sa_scr(p, None, None, xt, *shp, 0.5, p + 256, p + 512, None, sp, None) == L.SA_ERR_ARG
        assert lib.sa_last_error()
        assert lib.sa_scr_scratch_bytes(*shp, xt) == L.SA_ERR_ARG
    assert lib.sa_scr(p, None, None, L.SA_F32, 8, 8, 1, 0.5, None, p + 512, None, sp, None) == L.SA_ERR_ARG
    assert lib.sa_scr(None, None, None, L.SA_F32, 8, 8, 1, 0.5, p + 256, None, None, sp, None) == L.SA_ERR_ARG
    assert lib.sa_scr(p, None, None, L.SA_F32, 8, 8, 1, 0.5, p + 256, None, None, None, None) == L.SA_ERR_ARG
    assert lib.sa_scr(p, None, None, L.SA_F32, 8, 8, 1, 0.5, p, None, None, sp, None) == L.SA_ERR_ARG  # aliases a
    torch.cuda.synchronize()
    assert torch.equal(t, before)
    a, out = t[:64], t[64:128]
    with pytest.raises(ValueError):
        K.scr(a, None, None, (8, 8, 1), 0.5, out, scratch=s[:-8])  # scratch too small
    with pytest.raises(ValueError):
        K.scr(a, None, None, (8, 4, 1), 0.5, out, scratch=s)  # shape3 does not cover a
    with pytest.raises(ValueError):
        K.scr(torch.zeros(64), None, None, (8, 8, 1), 0.5, out, scratch=s)  # a host tensor
    with pytest.raises(TypeError):
        K.scr_scratch_bytes((8, 8, 1), torch.int64)
    torch.cuda.synchronize()
    assert torch.equal(t, before)
