"""sa_flame_stats_wide / sa_flame_combine_wide (17 to 64 clients) and
FlameAggregator(wide_clients="device") against the host form and the exact
statistics (tests/flame_oracle.py).  Sizes: around one tile of E elements, and
one case past STAT_BLOCKS tiles (a block of two tiles, an odd last tile)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import flame_oracle as O  # noqa: E402
from test_gpu_flame import _bits, _dev, _gamma, _get  # noqa: E402  (the narrow entries' test: the same helpers)
from test_gpu_flame import _put as _put_on  # noqa: E402
from sfl_amd import _lib as L  # noqa: E402
from sfl_amd import kernels as K  # noqa: E402
from sfl_amd.device import PYU, PYUObject  # noqa: E402
from sfl_amd.security.aggregation import FlameAggregator  # noqa: E402
from sfl_amd.security.aggregation import flame_aggregator as F  # noqa: E402

pytestmark = pytest.mark.gpu

E, STAT_BLOCKS = 128, 512  # sa_flame_wide.hip's kE and kStatBlocks
TYPES = ("float32", "float64")
CASES = sorted({(c, E + 1, t) for c in (17, 31, 32, 33, 48, 63, 64) for t in TYPES}
               | {(c, n, t) for c, t in ((17, "float64"), (33, "float32")) for n in (0, 1, 3, E - 1, E, E + 1, 4 * E + 5)})


def _put(a):
    return _put_on(a, _dev())


def _vectors(C, n, tname):
    rng = np.random.default_rng(7919 * C + n % 100003 + np.dtype(tname).itemsize)
    return [(rng.standard_normal(n) * rng.choice([0.01, 1.0, 30.0])).astype(tname) for _ in range(C)]


@functools.lru_cache(maxsize=None)
def _case(C, n, tname):
    """The clients' vectors, the host median, the exact statistics and the sums of their terms' magnitudes."""
    xs = _vectors(C, n, tname)
    g = F.median_host(np.stack(xs)) if n else np.zeros(0, tname)
    exact, mags = O.exact_stats([xs], [g])
    return xs, g, exact, mags


def _stats(xs_dev, n, C, tdt, stats=None, accumulate=False):
    dev = _dev()
    g = torch.empty(n, dtype=tdt, device=dev)
    scratch = torch.empty(K.flame_wide_scratch_bytes(n, C, tdt), dtype=torch.uint8, device=dev)
    if stats is None:
        stats = torch.full((K.flame_stat_count(C),), float("nan"), dtype=torch.float64, device=dev)
    K.flame_stats_wide(xs_dev, g, scratch, stats, accumulate=accumulate)
    return g, stats


def _within(label, err, bound):
    print(f"{label}: max |stat - reference| / bound = {float((err / np.where(bound > 0, bound, 1)).max()):.3e}")
    assert np.all(err <= bound)


def _check_combine(xs, xs_dev, g, g_host, C, n):
    """Scales that are no T values, a weight sum that is no power of two, clients 0, 1 and C - 1 dropped and then
    poisoned: combine_host's bits."""
    rng = np.random.default_rng(C + n)
    scales = rng.uniform(0.1, 0.999, C)
    weights = [float(v) for v in rng.integers(1, 50, C) * 2 + 1]
    keep = [i not in (0, 1, C - 1) for i in range(C)]
    W = float(np.asarray([w for w, k in zip(weights, keep) if k], np.float64).sum())
    assert W != 2.0 ** np.round(np.log2(W))
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=g.device)
    K.flame_combine_wide(xs_dev, scales, weights, keep, g, W, out)
    if n:
        # (one element: combine_host hands it to np.average, whose pairwise sum is the class's business; the entry's
        # sum in client order is combine_host's of the element twice)
        rep = 2 if n == 1 else 1
        want = F.combine_host([np.repeat(x, rep) for x in xs], np.repeat(g_host, rep), scales, weights, keep)[:n]
        assert np.array_equal(_bits(_get(out)), _bits(want))
        poisoned = [x if k else torch.full_like(x, float("nan")) for x, k in zip(xs_dev, keep)]
        out2 = torch.empty_like(out)
        K.flame_combine_wide(poisoned, scales, weights, keep, g, W, out2)
        assert torch.equal(out.view(torch.int64), out2.view(torch.int64))


@pytest.mark.parametrize("C,n,tname", CASES)
def test_stats_median_and_combine_against_the_host_form(C, n, tname):
    tdt = getattr(torch, tname)
    xs, g_host, exact, mags = _case(C, n, tname)
    xs_dev = [_put(x) for x in xs]
    g, stats = _stats(xs_dev, n, C, tdt)
    g2, stats2 = _stats(xs_dev, n, C, tdt)
    got = _get(stats)
    assert np.array_equal(_bits(_get(g)), _bits(g_host))
    # every statistic within gamma_n sum |t_k| of the exact sum (any order, with or without FMA; n == 0: zeros)
    _within(f"C={C} n={n} {tname}", np.abs(got - exact), _gamma(max(n, 1)) * mags * (1 + 1e-9))
    assert np.array_equal(_bits(got), _bits(_get(stats2))) and torch.equal(g.view(torch.uint8), g2.view(torch.uint8))
    _check_combine(xs, xs_dev, g, g_host, C, n)


def test_a_block_of_two_tiles_and_an_odd_last_tile():
    C, n, tname = 17, STAT_BLOCKS * E + E + 37, "float32"
    xs = _vectors(C, n, tname)
    g_host = F.median_host(np.stack(xs))
    xs_dev = [_put(x) for x in xs]
    g, stats = _stats(xs_dev, n, C, torch.float32)
    got = _get(stats)
    assert np.array_equal(_bits(_get(g)), _bits(g_host))
    # float64 numpy products: each side is within gamma_n of the exact sum
    X = np.stack(xs).astype(np.float64)
    D = (np.stack(xs) - g_host).astype(np.float64)
    iu = np.triu_indices(C)
    want = np.concatenate([(X @ X.T)[iu], (D * D).sum(1)])
    mags = np.concatenate([(np.abs(X) @ np.abs(X).T)[iu], (D * D).sum(1)])
    _within(f"C={C} n={n} {tname} (numpy)", np.abs(got - want), 2 * _gamma(n) * mags)
    assert np.array_equal(_bits(got), _bits(_get(_stats(xs_dev, n, C, torch.float32)[1])))
    _check_combine(xs, xs_dev, g, g_host, C, n)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("C", [17, 32, 33, 64])
def test_median_of_special_columns(C, tname):
    T, n = np.dtype(tname), E + 1
    big, tiny = np.finfo(T).max, np.finfo(T).smallest_subnormal
    rng = np.random.default_rng(C)
    st = rng.standard_normal((C, n)).astype(T)
    st[0, 1], st[C // 2, 2], st[C - 1, 3] = np.nan, -np.nan, np.nan
    st[:, 4], st[:, 5] = big, -big  # an even C: lo + hi overflows to inf
    st[:, 6], st[:, 7], st[:, 8] = np.inf, -np.inf, 1.5
    st[:, 9] = rng.permutation(np.array([-np.inf] * (C // 2) + [np.inf] * (C - C // 2), T))
    for col, negatives in ((10, C // 2), (11, C // 2 + 1), (E, C // 2)):  # -0 < +0 decides the middle
        st[:, col] = rng.permutation(np.array([-0.0] * negatives + [0.0] * (C - negatives), T))
    st[:, 12], st[:, 13] = np.arange(C), -np.arange(C)  # ascending and descending in client order
    st[:, 14] = rng.permutation(np.array([big, -big, tiny, -tiny] * 16, T)[:C])  # a sentinel compared as data
    st[:, 15] = rng.permutation(np.array([-big] * (C // 2 + 1) + [big] * (C - C // 2 - 1), T))
    st[:, 16] = rng.permutation(np.array([-big] * (C // 2 - 1) + [big] * (C - C // 2 + 1), T))
    want = F.median_host(st)
    g, _ = _stats([_put(r) for r in st], n, C, getattr(torch, tname))
    got = _get(g)
    assert np.isnan(got[1:4]).all() and got[4] == (np.inf if C % 2 == 0 else big)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("tname", TYPES)
def test_accumulate_and_unaligned_base_pointers(tname):
    dev, C, tdt = _dev(), 33, getattr(torch, tname)
    (xa, ga, ea, ma), (xb, gb, eb, mb) = _case(C, E - 1, tname), _case(C, 4 * E + 5, tname)
    na, nb = E - 1, 4 * E + 5
    da, db = [_put(x) for x in xa], [_put(x) for x in xb]

    def run():
        _, stats = _stats(da, na, C, tdt)
        return _get(_stats(db, nb, C, tdt, stats=stats, accumulate=True)[1])

    both = run()
    assert np.array_equal(_bits(both), _bits(run()))
    exact, _ = O.exact_stats([xa, xb], [ga, gb])
    _within(f"C={C} two layers {tname}", np.abs(both - exact), _gamma(na + nb) * (ma + mb) * (1 + 1e-9))
    # base pointers offset by one element: the same bits as the aligned copies
    shifted = []
    for x in db:
        base = torch.empty(nb + 1, dtype=tdt, device=dev)
        base[1:] = x
        shifted.append(base[1:])
        assert shifted[-1].data_ptr() % 16 != 0
    g = torch.empty(nb + 1, dtype=tdt, device=dev)[1:]
    scratch = torch.empty(K.flame_wide_scratch_bytes(nb, C, tdt), dtype=torch.uint8, device=dev)
    stats = torch.zeros(K.flame_stat_count(C), dtype=torch.float64, device=dev)
    K.flame_stats_wide(shifted, g, scratch, stats)
    g_al, stats_al = _stats(db, nb, C, tdt)
    assert np.array_equal(_bits(_get(g)), _bits(gb)) and torch.equal(g.view(torch.uint8), g_al.view(torch.uint8))
    assert np.array_equal(_bits(_get(stats)), _bits(_get(stats_al)))
    out = torch.empty(nb + 1, dtype=torch.float64, device=dev)[1:]
    K.flame_combine_wide(shifted, [0.3] * C, [3.0] * C, [True] * C, g, 3.0 * C, out)
    assert np.array_equal(_bits(_get(out)), _bits(F.combine_host(xb, gb, [0.3] * C, [3.0] * C, [True] * C)))


# ------------------------------------------------------------------ the class
def _planted(T, C=20):
    """tests/test_gpu_flame.py's planted case for 20 clients: a majority near a common base, two clients scaled up,
    three unrelated and sign-flipped, one noisy."""
    rng = np.random.default_rng(3)
    base = [rng.standard_normal(s) for s in ((1,), (257,), (E + 3,))]
    data = [[((1.5 if i in (4, 11) else 1.0) * b + (0.1 if i == 2 else 0.01) * rng.standard_normal(b.shape)).astype(T)
             for b in base] for i in range(C)]
    for i in (3, 9, 15):
        data[i] = [(-4 * rng.standard_normal(b.shape)).astype(T) for b in base]
    return data


@pytest.mark.parametrize("tname", TYPES)
def test_the_aggregator_on_twenty_device_clients(tname):
    dev = _dev()
    T, tdt, C = np.dtype(tname), getattr(torch, tname), 20
    data = _planted(T)
    weights = [float(v) for v in np.random.default_rng(5).integers(1, 60, C)]
    _, host = F.flame_host(data, weights)
    n = sum(a.size for a in data[0])
    # no edge of the distance graph is close enough to another for the statistics' rounding to swap them
    assert np.diff(np.unique(host["cosine_distances"][np.triu_indices(C, 1)])).min() > 1000 * 3 * _gamma(n)
    server, client = PYU("server", 0), PYU("client", 0)
    agg = FlameAggregator(server, wide_clients="device")
    out = agg.average([PYUObject(client, [_put(a) for a in d]) for d in data], axis=0, weights=weights).data
    rep = agg.last_report
    assert rep["wide_clients"] is True and rep["labels"] == host["labels"] and rep["labels"].count(-1) >= 3
    assert all(o.is_cuda and o.dtype == torch.float64 and o.shape == a.shape for o, a in zip(out, data[0]))
    for key in ("norms", "scales", "cosine_distances"):
        assert np.allclose(rep[key], host[key], rtol=1e-11, atol=1e-11), key
    # the decisions from the GPU's own statistics, the combine on the host: the same bits
    stats = None
    for l in range(3):
        _, stats = _stats([_put(d[l]) for d in data], data[0][l].size, C, tdt, stats=stats, accumulate=l > 0)
    mine = F.decide(_get(stats), C)
    keep = [lb == 0 for lb in mine["labels"]]
    for l in range(3):
        xs = [d[l] for d in data]
        want = F.combine_host(xs, F.median_host(np.stack(xs)), mine["scales"], weights, keep)
        assert np.array_equal(_bits(_get(out[l])), _bits(want)), l
    # a mixed upload: client 1 numpy arrays, client 2 CPU tensors, the others on the device
    mixed = [PYUObject(client, list(d) if i == 1 else [torch.from_numpy(a) if i == 2 else _put(a) for a in d])
             for i, d in enumerate(data)]
    out2 = FlameAggregator(server, wide_clients="device").average(mixed, axis=0, weights=weights).data
    for a, b in zip(out, out2):
        assert b.is_cuda and torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_bad_arguments_come_back_as_status_and_message():
    dev, n, C, server = _dev(), 64, 17, PYU("server", 0)
    data = [PYUObject(server, [torch.ones(8, device=dev) * i]) for i in range(65)]
    with pytest.raises(NotImplementedError, match="SA_FLAME_WIDE_MAX_CLIENTS"):
        FlameAggregator(server, wide_clients="device").average(data, axis=0)
    with pytest.raises(ValueError, match="wide_clients"):
        FlameAggregator(server, wide_clients="gpu")
    x = torch.ones(n, device=dev)
    g, out = torch.empty(n, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    scratch = torch.empty(K.flame_wide_scratch_bytes(n, 64, torch.float64), dtype=torch.uint8, device=dev)
    stats = torch.zeros(K.flame_stat_count(65), dtype=torch.float64, device=dev)
    xi, gi = torch.ones(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)

    def combine(xs, keep=True, median=g):
        c = len(xs)
        return lambda: K.flame_combine_wide(xs, [1.0] * c, [1.0] * c, [keep] * c, median, float(c), out)

    cases = [
        (lambda: K.flame_wide_scratch_bytes(n, 16, torch.float32), "n_clients must be in 17..64"),
        (lambda: K.flame_wide_scratch_bytes(n, 65, torch.float32), "n_clients must be in 17..64"),
        (lambda: K.flame_stats_wide([xi] * C, gi, scratch, stats), "SA_F32 or SA_F64"),
        (lambda: K.flame_stats_wide([x] * 16, g, scratch, stats), "n_clients must be in 17..64"),
        (lambda: K.flame_stats_wide([x] * 65, g, scratch, stats), "n_clients must be in 17..64"),
        (lambda: K.flame_stats_wide([x] * 16 + [None], g, scratch, stats), "client 16"),
        (lambda: K.flame_stats_wide([x] * 16 + [x.data_ptr() + 2], g, scratch, stats), "client 16"),
        (combine([xi] * C, median=gi), "SA_F32 or SA_F64"),
        (combine([x] * 16), "n_clients must be in 17..64"),
        (combine([x] * 65), "n_clients must be in 17..64"),
        (combine([x] * 16 + [None]), "client 16"),
        (combine([x] * 16 + [x.data_ptr() + 2]), "aligned"),
        (combine([x] * C, keep=False), "dropped"),
    ]
    for call, word in cases:
        with pytest.raises(L.SALibraryError, match=f"code {L.SA_ERR_ARG}: .*{word}"):
            call()
