"""sa_flame_stats / sa_flame_combine and FlameAggregator on the device against
the host form (sfl_amd/security/aggregation/flame_aggregator.py) and the exact
statistics (tests/flame_oracle.py).

Every array moves through hostpipe's pinned buffers (tests/gpu_copies.py): the
file adds no pageable DMA to the test process (DESIGN.md sections 7 and 13).

Sizes: around one tile (256) and one block (1,024), and 2^20 + 1,029: past
1,024 blocks x 1,024 elements, so a wave owns more than one tile and the last
wave is ragged.  Clients: odd and even counts, both sides of the one-pass /
two-pass boundary (8 | 9) and the limit (16)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import flame_oracle as O  # noqa: E402
import gpu_copies  # noqa: E402
from sfl_amd import _lib as L  # noqa: E402
from sfl_amd.security.aggregation import flame_aggregator as F  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 2**20 + 1029]
CLIENTS = [1, 2, 3, 4, 5, 8, 9, 16]
# every C at n = 1,025 in both types; every n at C = 3 (float64) and C = 8 (float32)
CASES = sorted({(c, 1025, t) for c in CLIENTS for t in ("float32", "float64")}
               | {(3, n, "float64") for n in SIZES} | {(8, n, "float32") for n in SIZES})


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _gamma(n):
    u = n * 2.0 ** -53
    return u / (1 - u)


def _put(a, dev):
    """A host array on the device through a pinned buffer (tests/gpu_copies.py): no pageable DMA."""
    return gpu_copies._dev(np.array(a) if np.size(a) == 0 else a)  # (an empty array: no copy is made)


def _get(t):
    """A device tensor's elements on the host, through a pinned buffer as well."""
    if t.numel() == 0:
        return np.empty(tuple(t.shape), str(t.dtype).replace("torch.", ""))
    return gpu_copies._host(t)


@functools.lru_cache(maxsize=None)
def _case(C, n, tname):
    """One case's inputs and references, computed once: the clients' vectors,
    the host median, the exact statistics and the sums of their terms' magnitudes."""
    T = np.dtype(tname)
    rng = np.random.default_rng(7919 * C + n % 100003 + T.itemsize)
    xs = [(rng.standard_normal(n) * rng.choice([0.01, 1.0, 30.0])).astype(T) for _ in range(C)]
    g = F.median_host(np.stack(xs)) if n else np.zeros(0, T)
    exact, mags = O.exact_stats([xs], [g])
    for a in xs + [g, exact, mags]:
        a.setflags(write=False)
    return xs, g, exact, mags


def _stats(K, dev, xs_dev, n, C, tdt, stats=None, accumulate=False):
    g = torch.empty(n, dtype=tdt, device=dev)
    scratch = torch.empty(K.flame_scratch_bytes(n, C, tdt), dtype=torch.uint8, device=dev)
    if stats is None:
        stats = torch.full((K.flame_stat_count(C),), float("nan"), dtype=torch.float64, device=dev)
    K.flame_stats(xs_dev, g, scratch, stats, accumulate=accumulate)
    return g, stats


@pytest.mark.parametrize("C,n,tname", CASES)
def test_stats_and_combine_against_the_host_form(C, n, tname):
    from sfl_amd import kernels as K

    dev = _dev()
    tdt = getattr(torch, tname)
    xs, g_host, exact, mags = _case(C, n, tname)
    xs_dev = [_put(x, dev) for x in xs]
    g, stats = _stats(K, dev, xs_dev, n, C, tdt)
    g2, stats2 = _stats(K, dev, xs_dev, n, C, tdt)
    got_g, got = _get(g), _get(stats)
    # the median: the host form's bits
    assert np.array_equal(_bits(got_g), _bits(g_host))
    # every statistic within gamma_n sum |t_k| of the exact sum (any order, with or without FMA)
    bound = _gamma(max(n, 1)) * mags * (1 + 1e-9)
    err = np.abs(got - exact)
    print(f"C={C} n={n} {tname}: max |stat - exact| / bound = {float((err / np.where(bound > 0, bound, 1)).max()):.3e}")
    assert np.all(err <= bound)
    if n == 0:
        assert np.all(got == 0)
    # the same bits on every run
    assert np.array_equal(_bits(got), _bits(_get(stats2))) and torch.equal(g.view(torch.uint8), g2.view(torch.uint8))
    # the combine: a scale that is no float32 value, a weight sum that is no power of two, a dropped client
    rng = np.random.default_rng(C + n)
    scales = rng.uniform(0.1, 0.999, C)
    scales[C - 1] = 1.0
    weights = [float(v) for v in rng.integers(1, 50, C) * 2 + 1]
    keep = [True] * C
    if C >= 3:
        keep[1] = False
    W = float(np.asarray([w for w, k in zip(weights, keep) if k], np.float64).sum())
    assert W != 2.0 ** np.round(np.log2(W)) or C == 1
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    K.flame_combine(xs_dev, scales, weights, keep, g, W, out)
    if n:
        want = F.combine_host(xs, g_host, scales, weights, keep)
        assert np.array_equal(_bits(_get(out)), _bits(want))
    if C >= 3 and n:
        # the dropped client's tensor is not read into the sum: poisoned (a valid address), the result stays
        poisoned = list(xs_dev)
        poisoned[1] = torch.full((n,), float("nan"), dtype=tdt, device=dev)
        out2 = torch.empty_like(out)
        K.flame_combine(poisoned, scales, weights, keep, g, W, out2)
        assert torch.equal(out.view(torch.int64), out2.view(torch.int64))


@pytest.mark.parametrize("tname", ["float32", "float64"])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 8, 9, 16])
def test_median_of_nan_overflow_and_signed_zero_columns(C, tname):
    from sfl_amd import kernels as K

    dev = _dev()
    T, n = np.dtype(tname), 1025
    rng = np.random.default_rng(C)
    st = rng.standard_normal((C, n)).astype(T)
    st[rng.integers(C), 5] = np.nan
    st[:, 6] = np.finfo(T).max  # an even C: lo + hi overflows to inf
    st[:, 7] = -np.finfo(T).max
    for col, negatives in ((300, C // 2), (301, C // 2 + 1), (1024, C // 2)):  # -0 < +0 decides the middle
        st[:, col] = rng.permutation(np.array([-0.0] * negatives + [0.0] * (C - negatives), T))
    st[rng.integers(C), 1023] = -np.nan
    want = F.median_host(st)
    g, _ = _stats(K, dev, [_put(r, dev) for r in st], n, C, getattr(torch, tname))
    got = _get(g)
    assert np.isnan(got[5]) and np.isnan(got[1023])
    assert np.array_equal(_bits(got), _bits(want))
    assert got[6] == (np.inf if C % 2 == 0 else np.finfo(T).max)
    assert not np.signbit(got[300]) and np.signbit(got[301]) and not np.signbit(got[1024])


@pytest.mark.parametrize("tname", ["float32", "float64"])
def test_accumulate_over_two_layers(tname):
    from sfl_amd import kernels as K

    dev = _dev()
    C, tdt = 5, getattr(torch, tname)
    (xa, ga, ea, ma), (xb, gb, eb, mb) = _case(C, 257, tname), _case(C, 1025, tname)
    da, db = [_put(x, dev) for x in xa], [_put(x, dev) for x in xb]

    def run():
        _, stats = _stats(K, dev, da, 257, C, tdt)
        _, stats = _stats(K, dev, db, 1025, C, tdt, stats=stats, accumulate=True)
        return _get(stats)

    both, again = run(), run()
    assert np.array_equal(_bits(both), _bits(again))
    sa = _get(_stats(K, dev, da, 257, C, tdt)[1])
    sb = _get(_stats(K, dev, db, 1025, C, tdt)[1])
    bound = _gamma(257 + 1025) * (ma + mb) * (1 + 1e-9)
    assert np.all(np.abs(both - (sa + sb)) <= bound)
    exact, _ = O.exact_stats([xa, xb], [ga, gb])
    assert np.all(np.abs(both - exact) <= bound)


@pytest.mark.parametrize("tname", ["float32", "float64"])
@pytest.mark.parametrize("C,n", [(3, 1025), (9, 2049)])
def test_unaligned_base_pointers_give_the_same_bits(C, n, tname):
    from sfl_amd import kernels as K

    dev = _dev()
    tdt = getattr(torch, tname)
    xs, g_host, _, _ = _case(C, n, tname)
    shifted = []
    for x in xs:
        base = torch.empty(n + 1, dtype=tdt, device=dev)
        base[1:] = _put(x, dev)
        shifted.append(base[1:])
        assert shifted[-1].data_ptr() % 16 != 0
    g = torch.empty(n + 1, dtype=tdt, device=dev)[1:]
    scratch = torch.empty(K.flame_scratch_bytes(n, C, tdt), dtype=torch.uint8, device=dev)
    stats = torch.zeros(K.flame_stat_count(C), dtype=torch.float64, device=dev)
    K.flame_stats(shifted, g, scratch, stats)
    assert np.array_equal(_bits(_get(g)), _bits(g_host))
    _, aligned = _stats(K, dev, [_put(x, dev) for x in xs], n, C, tdt)
    assert np.array_equal(_bits(_get(stats)), _bits(_get(aligned)))  # the same lane-to-element map
    out = torch.empty(n + 1, dtype=torch.float64, device=dev)[1:]
    K.flame_combine(shifted, [0.3] * C, [3.0] * C, [True] * C, g, 3.0 * C, out)
    want = F.combine_host(xs, g_host, [0.3] * C, [3.0] * C, [True] * C)
    assert np.array_equal(_bits(_get(out)), _bits(want))


# ------------------------------------------------------------------ the class
def _planted(T, C=5):
    """test_flame_host's planted case with layers of 1, 257 and 4,099 elements."""
    rng = np.random.default_rng(3)
    base = [rng.standard_normal(s) for s in ((1,), (257,), (4099,))]
    noise = {2: 0.1}
    data = [[((1.5 if i == 4 else 1.0) * b + noise.get(i, 0.01) * rng.standard_normal(b.shape)).astype(T) for b in base]
            for i in range(C)]
    data[3] = [(-4 * rng.standard_normal(b.shape)).astype(T) for b in base]
    return data


@pytest.mark.parametrize("tname", ["float32", "float64"])
def test_the_aggregator_on_device_tensors(tname):
    from sfl_amd import kernels as K
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import FlameAggregator

    dev = _dev()
    T, tdt, C = np.dtype(tname), getattr(torch, tname), 5
    data = _planted(T)
    weights = [40, 10, 30, 20, 50]
    server, client = PYU("server", 0), PYU("client", 0)
    agg = FlameAggregator(server)
    out = agg.average([PYUObject(client, [_put(a, dev) for a in d]) for d in data], axis=0, weights=weights).data
    rep = agg.last_report
    assert all(o.is_cuda and o.dtype == torch.float64 and o.shape == a.shape for o, a in zip(out, data[0]))
    # the decisions from the GPU's own statistics, the combine on the host: the same bits
    stats = None
    for l in range(3):
        _, stats = _stats(K, dev, [_put(d[l], dev) for d in data], data[0][l].size, C, tdt, stats=stats,
                          accumulate=l > 0)
    mine = F.decide(_get(stats), C)
    assert mine["labels"] == rep["labels"] == [0, 0, -1, -1, 0]
    keep = [lb == 0 for lb in mine["labels"]]
    for l in range(3):
        xs = [d[l] for d in data]
        want = F.combine_host(xs, F.median_host(np.stack(xs)), mine["scales"], weights, keep)
        assert np.array_equal(_bits(_get(out[l])), _bits(want)), l
    # every field of the report agrees with the all-host run; no edge of the distance graph is close enough to
    # another for the statistics' rounding to swap them: |d cd| <= 3 gamma_n (|G_ij| <= sum |t_k| <= sqrt(G_ii G_jj))
    _, host = F.flame_host(data, weights)
    n = sum(a.size for a in data[0])
    edges = np.unique(host["cosine_distances"][np.triu_indices(C, 1)])
    assert np.diff(edges).min() > 1000 * 3 * _gamma(n)
    assert host["labels"] == rep["labels"]
    for key in ("norms", "scales", "cosine_distances"):
        assert np.allclose(rep[key], host[key], rtol=1e-11, atol=1e-11), key
    assert abs(rep["threshold"] - host["threshold"]) <= 1e-11 * host["threshold"]
    assert rep["scales"][4] < 0.5
    # a mixed upload: client 1 numpy arrays, client 2 CPU tensors (moved by PYUObject.to), the others on the device
    mixed = [PYUObject(client, list(d) if i == 1 else [torch.from_numpy(a) if i == 2 else _put(a, dev) for a in d])
             for i, d in enumerate(data)]
    out2 = FlameAggregator(server).average(mixed, axis=0, weights=weights).data
    for a, b in zip(out, out2):
        assert b.is_cuda and torch.equal(a.view(torch.int64), b.view(torch.int64))


# ------------------------------------------------------------------ refusals
def test_seventeen_clients_on_the_device_are_refused():
    from sfl_amd.device import PYU, PYUObject
    from sfl_amd.security.aggregation import FlameAggregator

    dev = _dev()
    server = PYU("server", 0)
    data = [PYUObject(server, [torch.ones(8, device=dev) * i]) for i in range(17)]
    with pytest.raises(NotImplementedError, match="16"):
        FlameAggregator(server).average(data, axis=0)


def test_bad_arguments_come_back_as_status_and_message():
    from sfl_amd import kernels as K

    dev = _dev()
    n = 64
    x = torch.ones(n, device=dev)
    g, out = torch.empty(n, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    scratch = torch.empty(K.flame_scratch_bytes(n, 16, torch.float64), dtype=torch.uint8, device=dev)
    stats = torch.zeros(K.flame_stat_count(17), dtype=torch.float64, device=dev)
    xi, gi = torch.ones(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    cases = [
        (lambda: K.flame_stats([xi, xi], gi, scratch, stats), "SA_F32 or SA_F64"),
        (lambda: K.flame_stats([], g, scratch, stats), "n_clients must be in 1..16"),
        (lambda: K.flame_stats([x] * 17, g, scratch, stats), "n_clients must be in 1..16"),
        (lambda: K.flame_stats([x, None], g, scratch, stats), "client 1"),
        (lambda: K.flame_stats([x, x.data_ptr() + 2], g, scratch, stats), "client 1"),
        (lambda: K.flame_combine([xi, xi], [1.0] * 2, [1.0] * 2, [True] * 2, gi, 2.0, out), "SA_F32 or SA_F64"),
        (lambda: K.flame_combine([], [], [], [], g, 2.0, out), "n_clients must be in 1..16"),
        (lambda: K.flame_combine([x] * 17, [1.0] * 17, [1.0] * 17, [True] * 17, g, 17.0, out), "n_clients must be in 1..16"),
        (lambda: K.flame_combine([x, None], [1.0] * 2, [1.0] * 2, [True] * 2, g, 2.0, out), "client 1"),
        (lambda: K.flame_combine([x, x.data_ptr() + 2], [1.0] * 2, [1.0] * 2, [True] * 2, g, 2.0, out), "aligned"),
        (lambda: K.flame_combine([x, x], [1.0] * 2, [1.0] * 2, [False] * 2, g, 2.0, out), "dropped"),
    ]
    for call, word in cases:
        with pytest.raises(L.SALibraryError, match=f"code {L.SA_ERR_ARG}: .*{word}"):
            call()
