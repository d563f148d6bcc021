"""Structure-wise pruning on the CPU: the tests' numpy restatement
(tests/scr_oracle.py) against what the reference's own SCRSparse dropped
(tests/golden/scr_reference.npz, made by tests/golden/make_scr_golden.py),
and the product's host path (sfl_amd.utils.compressor.scr_step / SCRSparse)
against both, bit for bit; then the cases numpy settles by IEEE arithmetic,
and the decisive-element cases (DECISIVE), whose sums are exact in every
order and sit on their thresholds; tests/test_gpu_scr.py runs those on the
device."""
import os

import numpy as np
import pytest
import torch

import scr_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scr_reference.npz")
IDS = ["f32", "f64"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def _unpack(packed, n):
    return np.unpackbits(packed)[:n].astype(bool)


def _reference_output(u, rows, cols):
    """What the reference leaves of ``u``: the recorded rows and columns set to 0.0."""
    out = u.copy().reshape(so.view3(u.shape))
    out[rows] = 0.0
    out[:, cols] = 0.0
    return out.reshape(u.shape)


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", so.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_and_host_path_match_the_reference_fixture(golden, dt, shape):
    from sfl_amd.utils import compressor as Cz

    for thr in so.THRESHOLDS:
        key = so.case_key(dt, shape, thr)
        u = so.case_input(golden[key + "_seed"], shape, dt)
        R, C, _ = so.view3(shape)
        rows_ref, cols_ref = _unpack(golden[key + "_rows"], R), _unpack(golden[key + "_cols"], C)
        rows, cols, r0, r1 = so.drop_flags(u, thr)
        assert np.array_equal(rows, rows_ref) and np.array_equal(cols, cols_ref), key
        assert so.margin(r0, r1, thr) >= so.MIN_MARGIN, key  # the fixture alone stays clear of its thresholds
        want = _reference_output(u, rows_ref, cols_ref)
        sparse, res = so.apply(u, rows, cols)
        assert _same(sparse, want), key
        keep = u.copy()
        got, got_res = Cz.scr_step(u, None, None, thr)
        assert _same(got, want) and _same(got_res, res), key
        (again,) = Cz.SCRSparse(thr)([u])
        assert _same(again, want) and again is not u and _same(u, keep), key


def test_fixture_drops_some_but_not_all_at_the_middle_thresholds(golden):
    for dt in so.DTYPES:
        for thr in (0.3, 0.8):
            key = so.case_key(dt, (65, 257), thr)
            rows, cols = _unpack(golden[key + "_rows"], 65), _unpack(golden[key + "_cols"], 257)
            assert 0 < rows.sum() < 65 and 0 < cols.sum() < 257, key


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
def test_operands_and_residual(dt):
    from sfl_amd.utils import compressor as Cz

    a, b, r = (so.case_input(s, (65, 33, 3, 3), dt) for s in (1, 2, 3))
    for bb, rr in ((b, None), (b, r), (None, None), (None, r)):
        want = so.scr(a, bb, rr, 0.3)
        got = Cz.scr_step(a, bb, rr, 0.3)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
        u = so.form(a, bb, rr)
        assert np.array_equal(got[0] + got[1], u)  # payload + dropped part = the dense update
        assert Cz.scr_step(a, bb, rr, 0.3, want_res=False)[1] is None
    t = Cz.scr_step(torch.from_numpy(a), torch.from_numpy(b), None, 0.3)  # CPU tensors give CPU tensors
    assert isinstance(t[0], torch.Tensor) and _same(t[0].numpy(), so.scr(a, b, None, 0.3)[0])


def tie_rows(dt):
    """Row sums 4, 2, 1 (small integers: exact in any order), threshold 0.5:
    the rows with ratio 0.5 and 0.25 go.  On the survivor the columns sum to
    2, 1, 1, 0: ratios 1, 0.5, 0.5, 0, so the last three go."""
    u = np.array([[2, -1, 1, 0], [1, 0, -1, 0], [0, 1, 0, 0]], dtype=dt)
    want = np.array([[2, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=dt)
    return u, 0.5, [False, True, True], [False, True, True, True], want


def tie_cols(dt):
    """No row at its threshold (sums 8, 6; ratio 0.75 > 0.5); the survivors'
    columns sum to 8, 4, 2: the column at exactly 0.5 goes with the one below."""
    u = np.array([[4, -2, 2], [4, 2, 0]], dtype=dt)
    want = np.array([[4, 0, 0], [4, 0, 0]], dtype=dt)
    return u, 0.5, [False, False], [False, True, True], want


def tie_conv(dt):
    """The rank-4 form of tie_rows: filters sum to 4, 2, 1 over (I, H, W)."""
    u = np.zeros((3, 2, 1, 2), dtype=dt)
    u[0] = [[[2, -1]], [[1, 0]]]
    u[1] = [[[1, 0]], [[-1, 0]]]
    u[2] = [[[0, 1]], [[0, 0]]]
    want = np.zeros_like(u)
    want[0, 0] = [[2, -1]]  # channels of the survivor: 3 and 1 -> ratio 1/3 goes
    return u, 0.5, [False, True, True], [False, True], want


TIES = (tie_rows, tie_cols, tie_conv)


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
@pytest.mark.parametrize("make", TIES, ids=lambda f: f.__name__)
def test_exact_threshold_ties(dt, make):
    from sfl_amd.utils import compressor as Cz

    u, thr, rows_want, cols_want, want = make(dt)
    sparse, res, rows, cols = so.scr(u, thr=thr)
    assert rows.tolist() == rows_want and cols.tolist() == cols_want
    assert _same(sparse, want)
    got = Cz.scr_step(u, None, None, thr)
    assert _same(got[0], want) and _same(got[1], res)


# --- decisive-element cases: the float64 sums themselves, at margin 0 ---------
#
# Every element is an integer multiple of q = 2^-20 of magnitude at most 2^10
# and exact in float32, so a structure's sum of magnitudes is an integer far
# below 2^53 in units of q (2^32 at most on the decided axis): every float64
# order of adding gives the same bits, and host and device divide the same two
# doubles.  That makes margin 0 legal: at threshold 0.5 the largest structure
# sums to S = 2^12 and every other one to S/2 + q (kept, because of one
# element q), S/2 (dropped on the tie), S/2 - q or S/2 - d (dropped).  A sum
# that loses an element, adds a foreign one or is kept in float32 lands on the
# other side.  A case's twin has the decisive q element +0: its structure is
# at the tie and goes.
Q = 2.0 ** -20
S_UNITS = 1 << 32  # S in units of q
HALF = S_UNITS >> 1
D_UNITS = 1 << 6  # d = 2^-14
THR = 0.5
KEPT, TIE, BELOW, BELOW_D, MAX = range(5)
_TARGET = {KEPT: HALF + 1, TIE: HALF, BELOW: HALF - 1, BELOW_D: HALF - D_UNITS, MAX: S_UNITS}


def _fill(rng, targets, n):
    """int64 [len(targets), n], all positive, row i summing to targets[i]
    exactly; entries of a row lie around its mean (pairs mean + x, mean - x)
    with two closing entries at random places, and every entry has few enough
    significant bits for float32."""
    t = np.asarray(targets, np.int64)
    mean = t // n
    sh = max(0, int(4 * mean.max()).bit_length() - 24)  # entries up to about 2 * mean keep 24 bits
    m = (mean >> sh) << sh
    out = np.empty((len(t), n), np.int64)
    pairs = (n - 2) // 2
    x = rng.integers(0, ((m >> (sh + 1)) + 1)[:, None], (len(t), pairs)) << sh  # up to mean / 2
    out[:, 0:2 * pairs:2] = m[:, None] + x
    out[:, 1:2 * pairs:2] = m[:, None] - x
    out[:, 2 * pairs:n - 2] = m[:, None]
    rest = t - out[:, :n - 2].sum(axis=1)  # about 2 * mean
    low = rest & ((1 << sh) - 1)
    low[low == 0] = 1 << sh
    out[:, n - 2], out[:, n - 1] = rest - low, low
    assert (out > 0).all() and np.array_equal(out.sum(axis=1), t)
    return rng.permuted(out, axis=1)


def _structures(rng, kinds, special, n, zero_at):
    """int64 [len(kinds), n] of magnitudes in units of q: structure i sums to
    its kind's target, and its entry ``special[i]`` is q alone for a KEPT
    structure (the element that keeps it), 0 for structure ``zero_at``, and
    an ordinary entry otherwise."""
    kinds = np.asarray(kinds)
    target = np.array([_TARGET[k] for k in kinds], np.int64)
    part = target // n
    own = np.where(kinds == KEPT, 1, np.int64(1) << (np.frexp(part.astype(np.float64))[1] - 1))
    own[zero_at] = 0
    assert kinds[zero_at] == TIE
    out = np.zeros((len(kinds), n), np.int64)
    mask = np.ones(out.shape, bool)
    mask[np.arange(len(kinds)), special] = False
    out[mask] = _fill(rng, target - own, n - 1).ravel()
    out[np.arange(len(kinds)), special] = own
    assert np.array_equal(out.sum(axis=1), target)
    return out


def _values(rng, units, minus_zero):
    """float64 of units * q with random signs and -0.0 at ``minus_zero``;
    checked: at most 2^10, exact in float32."""
    assert units[minus_zero] == 0
    v = units.astype(np.float64) * Q * rng.choice((-1.0, 1.0), units.shape)
    v[minus_zero] = -0.0
    assert np.abs(v).max() <= 2.0 ** 10
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)  # float32 holds every element
    assert np.array_equal(np.abs(v) / Q, units)  # and it is the multiple of q that was meant
    return v


def _pattern(count, fixed, groups):
    """Kinds of ``count`` structures; ``fixed`` (index: kind) is given.  The
    others alternate dropped and kept, the dropped ones tie and S/2 - q in
    turn.  With ``groups`` the first 40 repeat kept, kept, kept, dropped,
    kept instead, so that an aligned group of four has its one dropped member
    at each of the four places in turn (and some groups none).  The first tie
    holds the -0.0 and the first S/2 - q becomes the S/2 - d one."""
    free = [j for j in range(count) if j not in fixed]
    kinds, drops = [KEPT] * count, 0
    for i, j in enumerate(free):
        if (j % 5 == 3) if groups and j < 40 else (i % 2 == 0):
            kinds[j] = (TIE, BELOW)[drops % 2]
            drops += 1
    for j, k in fixed.items():
        kinds[j] = k
    zero_at = next(j for j in free if kinds[j] == TIE)
    kinds[next(j for j in free if kinds[j] == BELOW)] = BELOW_D
    return kinds, zero_at


_built = {}


def decisive_rows(shape, row, pos):
    """Row sums.  (u, index): every row within q / S of the threshold, row
    ``row`` kept only by the q at position ``pos`` of its ``L``; ``index`` is
    that element's.  float64, cast by the caller."""
    key = ("rows", shape, row, pos)
    if key not in _built:
        R, C, K = so.view3(shape)
        L = C * K
        rng = np.random.default_rng([R, L, row, pos])
        kinds, zero_at = _pattern(R, {row: KEPT, (row + R // 2) % R: MAX}, False)
        special = (np.arange(R) * 977 + 13) % L
        special[row] = pos
        units = _structures(rng, kinds, special, L, zero_at)
        v = _values(rng, units, (zero_at, special[zero_at]))
        _built[key] = v.reshape(shape), np.unravel_index(row * L + pos, shape)
    return _built[key]


def decisive_cols(shape, row, col, inner=0):
    """Column sums over the kept rows.  (u, index, gone, ties): two rows, one
    in the first slab of rows and one in the last, are far below the row
    threshold and go; over the others every column is within q / S of the
    threshold, column ``col`` kept only by the q at ``[row, col, inner]``.
    The rows in ``gone`` hold 2q in each column of ``ties`` and nothing else:
    a column sum that counted them would keep those columns."""
    key = ("cols", shape, row, col, inner)
    if key not in _built:
        R, C, K = so.view3(shape)
        gone = (0 if row == 1 else 1, R - 2 if row == R - 1 else R - 1)
        kept = np.setdiff1d(np.arange(R), gone)
        n = len(kept) * K
        rng = np.random.default_rng([R, C, K, row, col, inner])
        kinds, zero_at = _pattern(C, {col: KEPT, C // 2 + (col == C // 2): MAX}, True)
        special = (np.arange(C) * 977 + 13) % n
        special[col] = int(np.searchsorted(kept, row)) * K + inner
        units = _structures(rng, kinds, special, n, zero_at)
        u3 = np.zeros((R, C, K), np.int64)
        u3[kept] = units.reshape(C, len(kept), K).transpose(1, 0, 2)
        ties = np.flatnonzero(np.asarray(kinds) == TIE)
        for g in gone:
            u3[g, ties, ties % K] = 2
        zero = (kept[special[zero_at] // K], zero_at, special[zero_at] % K)
        v = _values(rng, u3, zero)
        _built[key] = v.reshape(shape), np.unravel_index((row * C + col) * K + inner, shape), gone, ties
    return _built[key]


def _row_positions(L):
    return sorted({p for p in (0, 3, 4, 255, 256, 2047, 2048, L - 2, L - 1) if 0 <= p < L})


def _row_cases(shape, rows):
    """The decisive q at each position of the list, the decisive row cycling
    through ``rows``."""
    _, C, K = so.view3(shape)
    return [(rows[i % len(rows)], p) for i, p in enumerate(_row_positions(C * K))]


# (kind, shape): the arguments of decisive_rows / decisive_cols, one per case.
# Which launch geometry each shape reaches is listed in DESIGN.md section 13.
DECISIVE = {
    ("rows", (8, 40)): _row_cases((8, 40), (0, 7, 3)),
    ("rows", (8, 300)): _row_cases((8, 300), (0, 7, 3)),
    ("rows", (6, 4100)): _row_cases((6, 4100), (0, 5, 2)),
    ("rows", (300, 2049)): _row_cases((300, 2049), (1, 255, 256, 299)),
    ("rows", (6, 260, 3, 3)): _row_cases((6, 260, 3, 3), (0, 5, 2)),
    ("rows", (5, 229, 3, 3)): _row_cases((5, 229, 3, 3), (0, 4, 2)),
    ("cols", (4099, 33)): [(0, 0), (2, 32), (3, 31), (4097, 7), (4098, 32)],
    ("cols", (1100, 2052)): [(0, 0), (1, 1023), (1098, 1024), (1099, 2047), (0, 2048), (1099, 2051)],
    ("cols", (2100, 12, 3, 3)): [(0, 0, 0), (2099, 0, 8), (0, 11, 8), (2099, 11, 0)],
    ("cols", (6, 260, 3, 3)): [(5, 259, 8), (2, 113, 4)],
}
DECISIVE_IDS = [f"{kind}-{'x'.join(map(str, shape))}" for kind, shape in DECISIVE]


def decisive(kind, shape, where, dt):
    """(u, twin, axis, structure, gone, ties) of one case in type ``dt``:
    ``structure`` of ``axis`` (0 rows, 1 columns) is kept in ``u`` and dropped
    in ``twin``, which is ``u`` with the decisive element +0."""
    if kind == "rows":
        v, index = decisive_rows(shape, *where)
        axis, gone, ties = 0, (), np.zeros(0, np.int64)
    else:
        v, index, gone, ties = decisive_cols(shape, *where)
        axis = 1
    u = v.astype(dt)
    assert abs(u[index]) == Q
    twin = u.copy()
    twin[index] = 0.0
    return u, twin, axis, index[axis], gone, ties


def _sums(u, dropped_rows=None, order=None, acc=np.float64):
    """The sums of magnitudes per row (``dropped_rows`` None) or per column
    over the other rows, added one after the other in ``acc`` along
    ``order(n)`` (None: as they lie)."""
    u3 = np.abs(u.reshape(so.view3(u.shape)))
    x = u3.reshape(len(u3), -1) if dropped_rows is None else \
        u3[~dropped_rows].transpose(1, 0, 2).reshape(u3.shape[1], -1)
    if order is not None:
        x = x[:, order(x.shape[1])]
    return np.cumsum(x, axis=1, dtype=acc)[:, -1].astype(np.float64)


def _flags(u, order=None, acc=np.float64, leak=False):
    """so.drop_flags at THR with the sums restated by _sums; with ``leak``
    the dropped rows are counted in the column sums."""
    s0 = _sums(u, None, order, acc)
    rows = s0 / np.max(s0) <= THR
    s1 = _sums(u, np.zeros_like(rows) if leak else rows, order, acc)
    return rows, s1 / np.max(s1) <= THR, s0, s1


def _each_decisive(kind, shape):
    for where in DECISIVE[kind, shape]:
        for dt in so.DTYPES:
            yield (where, np.dtype(dt).name), decisive(kind, shape, where, dt)


@pytest.mark.parametrize("kind,shape", list(DECISIVE), ids=DECISIVE_IDS)
def test_decisive_sums_are_exact_in_every_order(kind, shape):
    """The exactness claim: forward, reversed and shuffled float64 sums have
    the same bits as numpy's pairwise ones and as integer arithmetic."""
    shuffle = np.random.default_rng(5).permutation
    for key, (u, twin, _, _, _, _) in _each_decisive(kind, shape):
        for x in (u, twin):
            rows, cols, r0, r1 = so.drop_flags(x, THR)
            units = np.rint(np.abs(x.astype(np.float64)) / Q).astype(np.int64).reshape(so.view3(shape))
            exact0 = units.sum(axis=(1, 2))
            exact1 = units[~rows].sum(axis=(0, 2))
            assert max(exact0.max(), exact1.max()) < 2 ** 53, key
            assert _same(r0, exact0 / np.float64(exact0.max())) and _same(r1, exact1 / np.float64(exact1.max())), key
            for order in (None, lambda n: np.arange(n)[::-1], shuffle):
                got = _flags(x, order)
                assert np.array_equal(got[0], rows) and np.array_equal(got[1], cols), key
                assert _same(got[2], exact0 * Q) and _same(got[3], exact1 * Q), key


@pytest.mark.parametrize("kind,shape", list(DECISIVE), ids=DECISIVE_IDS)
def test_decisive_cases_sit_on_their_thresholds(kind, shape):
    """Every structure of the decided axis is the maximum or within q / S of
    the threshold; the twin differs in the decisive structure's flag alone; a
    float32 accumulation changes a flag in every case, and so does a column
    sum that counts the dropped rows."""
    for key, (u, twin, axis, j, gone, ties) in _each_decisive(kind, shape):
        rows, cols, r0, r1 = so.drop_flags(u, THR)
        rows_t, cols_t, _, _ = so.drop_flags(twin, THR)
        near = (r0, r1)[axis]
        assert np.all((near == 1.0) | (np.abs(near - THR) <= D_UNITS / S_UNITS)), key
        assert abs(near[j] - THR) == 1.0 / S_UNITS and np.count_nonzero(near == THR) >= 1, key
        # (a row that goes leaves the column sums, so in the row form the twin's columns are its own)
        flags, flags_t = np.concatenate([rows, cols]), np.concatenate([rows_t, cols_t])
        at, end = j + (len(rows) if axis else 0), len(flags) if axis else len(rows)
        assert not flags[at] and flags_t[at], key
        assert np.array_equal(np.delete(flags[:end], at), np.delete(flags_t[:end], at)), key
        assert np.signbit(u[u == 0]).any() and (u < 0).any() and (u > 0).any(), key
        rows32, cols32, _, _ = _flags(u, acc=np.float32)
        assert not np.array_equal(np.concatenate([rows32, cols32]), flags), key
        if axis:
            assert np.flatnonzero(rows).tolist() == list(gone) and cols[ties].all(), key
            leaky = _flags(u, leak=True)
            assert np.array_equal(leaky[0], rows) and not leaky[1][ties].any(), key
        if axis and len(shape) == 2 and shape[1] % 4 == 0:  # four flags read as one word: one set byte, each place
            groups = cols.reshape(-1, 4)
            alone = groups[groups.sum(axis=1) == 1]
            assert alone.any(axis=0).all(), key


@pytest.mark.parametrize("kind,shape", list(DECISIVE), ids=DECISIVE_IDS)
def test_host_path_decides_the_decisive_cases_alike(kind, shape):
    from sfl_amd.utils import compressor as Cz

    for key, (u, twin, _, _, _, _) in _each_decisive(kind, shape):
        for x in (u, twin):
            want = so.scr(x, thr=THR)
            got = Cz.scr_step(x, None, None, THR)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), key


def specials(dt):
    """(name, u, thr, expected sparse) with the expectation worked out from
    numpy's own arithmetic on the reference's steps."""
    base = so.case_input(77, (6, 5), dt)
    out = []
    u = base.copy()
    u[2, 3] = np.nan  # max is NaN: every ratio NaN, nothing goes
    out.append(("one_nan", u, 0.8, u.copy()))
    u = base.copy()
    u[1, 2] = np.inf  # inf/inf = NaN keeps row 1; finite rows have ratio 0; then column 2 alone is inf
    want = np.zeros_like(u)
    want[1, 2] = np.inf
    out.append(("one_inf", u, 0.0, want))
    out.append(("all_zero", np.zeros((6, 5), dt), 0.8, np.zeros((6, 5), dt)))  # 0/0 = NaN: nothing goes
    u = np.array([[4, -0.0, 1], [1, -0.0, -0.0], [4, 3, -0.0]], dtype=dt)  # row 1 goes (1/7), then column 2 (1/8)
    want = np.array([[4, -0.0, 0.0], [0.0, 0.0, 0.0], [4, 3, 0.0]], dtype=dt)
    out.append(("negative_zero", u, 0.25, want))
    return out


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
def test_special_values_follow_numpy(dt):
    from sfl_amd.utils import compressor as Cz

    for name, u, thr, want in specials(dt):
        # numpy's outcome by the reference's own steps, in float64
        ref = u.copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            s0 = np.sum(np.abs(ref), axis=1, dtype=np.float64)
            ref[np.argwhere(s0 / np.max(s0) <= thr)[:, 0], :] = 0.0
            s1 = np.sum(np.abs(ref), axis=0, dtype=np.float64)
            ref[:, np.argwhere(s1 / np.max(s1) <= thr)[:, 0]] = 0.0
        assert _same(ref, want), name
        sparse, res, _, _ = so.scr(u, thr=thr)
        assert _same(sparse, want), name
        got = Cz.scr_step(u, None, None, thr)
        assert _same(got[0], want) and _same(got[1], res), name
        kept = _bits(sparse) == _bits(u)
        assert np.all(np.isnan(res[kept & ~np.isfinite(u)])) and not _bits(res[kept & np.isfinite(u)]).any(), name


@pytest.mark.parametrize("dt", so.DTYPES, ids=IDS)
def test_negative_threshold_drops_nothing_and_large_drops_rows_only(dt):
    u = so.case_input(5, (8, 3, 3, 3), dt)
    sparse, res, rows, cols = so.scr(u, thr=-1.0)
    assert not rows.any() and not cols.any() and _same(sparse, u)
    sparse, res, rows, cols = so.scr(u, thr=2.0)
    assert rows.all() and not cols.any() and not _bits(sparse).any() and _same(res, u)


def test_other_ranks_pass_through_and_inputs_stay():
    from sfl_amd.utils import compressor as Cz

    rng = np.random.default_rng(1)
    for shape in ((), (7,), (2, 3, 4), (2, 1, 2, 1, 3)):
        u = np.asarray(rng.standard_normal(shape), dtype=np.float32)
        keep = u.copy()
        sparse, res = Cz.scr_step(u, None, None, 2.0)
        assert _same(sparse, u) and sparse is not u and not _bits(res).any() and _same(u, keep)
    a, b, r = (so.case_input(s, (7, 5), np.float32) for s in (1, 2, 3))
    keep = [x.copy() for x in (a, b, r)]
    Cz.scr_step(a, b, r, 0.8)
    Cz.SCRSparse(0.8)([a, b])
    assert all(_same(x, k) for x, k in zip((a, b, r), keep))
    assert Cz.SCRSparse(0.8).name == "SCR"
    empty = np.zeros((0, 4), np.float32)
    sparse, res = Cz.scr_step(empty, None, None, 0.5)
    assert sparse.shape == (0, 4) and res.shape == (0, 4)


def test_integer_entry_keeps_its_dtype():
    from sfl_amd.utils import compressor as Cz

    u = np.array([[4, -2, 2], [1, 0, 0], [4, 2, 0]], dtype=np.int64)  # row 1: 1/8; then columns 8, 4, 2
    sparse, res = Cz.scr_step(u, None, None, 0.3)
    assert sparse.dtype == np.int64 and res.dtype == np.int64
    assert sparse.tolist() == [[4, -2, 0], [0, 0, 0], [4, 2, 0]]
    assert np.array_equal(sparse + res, u)
    counter = np.array(7, dtype=np.int64)  # num_batches_tracked
    sparse, res = Cz.scr_step(counter, None, None, 0.3)
    assert sparse.dtype == np.int64 and sparse == 7 and res == 0
