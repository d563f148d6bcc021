"""``SparsePlainAggregator`` over device ``SparseCOO``s (one ``sa_coo_axpy``
per party, ``sa_coo_finish``): equal to the host aggregator on the same
payloads bit for bit, and to numpy over the decoded arrays
(tests/coo_oracle.py) with the sign of a zero apart."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import coo_oracle as co  # noqa: E402
from gpu_copies import DEV, _bits, _host  # noqa: E402
from sfl_amd.device import PYU, PYUObject  # noqa: E402
from sfl_amd.security import SparsePlainAggregator  # noqa: E402
from sfl_amd.utils.sparse import sparse_encode  # noqa: E402
from test_sparse_coo import LAYERS as HOST_LAYERS  # noqa: E402

pytestmark = pytest.mark.gpu
LAYERS = HOST_LAYERS + ((65537,),)  # 257 waves' worth: more than one block of entries per party
KS = (1, 2, 3, 8, 9)
DTYPES = (np.float32, np.float64)
IDS = ["f32", "f64"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _parties(K, dt, support, seed=0):
    """K per-layer lists (test_sparse_coo._parties over this file's LAYERS):
    overlapping, disjoint or empty supports; no NaN and no inf."""
    rng = np.random.default_rng(seed + K)
    out = []
    for k in range(K):
        layers = []
        for shape in LAYERS:
            n = int(np.prod(shape))
            v = (rng.standard_normal(n) * 10.0 ** float(rng.integers(-3, 4))).astype(dt)
            if support == "overlap":
                keep = rng.random(n) < 0.5
            elif support == "disjoint":
                keep = np.arange(n) % K == k
            elif support == "one_empty":
                keep = (rng.random(n) < 0.5) & (k != K // 2)
            else:
                keep = np.zeros(n, dtype=bool)
            layers.append(np.where(keep, v, dt(0)).reshape(shape))
        out.append(layers)
    return out


def _weights(kind, K, dt):
    if kind == "int":
        return [32 + 7 * k for k in range(K)]  # A = float64
    if kind == "f32":
        return list((np.random.default_rng(K).random(K) + 1.0).astype(np.float32))  # on float32 data: A = float32
    return None


def _objs(parties, where):
    """One PYUObject per party; ``where(k)`` says whether party k's entries are on the device."""
    out = []
    for k, layers in enumerate(parties):
        coos = sparse_encode(layers)
        out.append(PYUObject(PYU(f"p{k}", None), [c.to(DEV) for c in coos] if where(k) else coos))
    return out


def _calls(dt):
    yield "sum", None
    yield "average", None
    yield "average", "int"
    if dt == np.float32:
        yield "average", "f32"


def _compare(got, host, dense_ref, what):
    for li, (g, h, r) in enumerate(zip(got, host, dense_ref)):
        if LAYERS[li] == (1,):  # at most one element: numpy itself, on the host
            assert isinstance(g, np.ndarray) and co.same_bits(g, r), (what, li)
            continue
        assert isinstance(g, torch.Tensor) and g.is_cuda and tuple(g.shape) == LAYERS[li], (what, li)
        g = _host(g)
        assert not np.isnan(r).any() and not np.isinf(r).any()  # every element is compared by bits
        assert g.dtype == h.dtype and np.array_equal(_bits(g), _bits(h)), (what, li)
        assert co.same_bits(g, r), (what, li)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("support", ["overlap", "disjoint", "one_empty", "empty"])
@pytest.mark.parametrize("K", KS)
def test_device_sum_equals_the_host_aggregator_and_numpy(K, support, dt):
    agg = SparsePlainAggregator(PYU("server", None))
    parties = _parties(K, dt, support)
    on_dev, on_host = _objs(parties, lambda k: True), _objs(parties, lambda k: False)
    for call, wk in _calls(dt):
        w = _weights(wk, K, dt)
        kw = {} if call == "sum" else {"weights": w}
        got = getattr(agg, call)(on_dev, axis=0, **kw).data
        host = getattr(agg, call)(on_host, axis=0, **kw).data
        ref = [co.total([p[li] for p in parties], axis=0) if call == "sum" else
               co.average([p[li] for p in parties], axis=0, weights=w) for li in range(len(LAYERS))]
        if wk == "f32":
            assert all(h.dtype == np.float32 for h in host)  # the accumulator stayed float32
        _compare(got, host, ref, (call, wk))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_mixed_list_gives_the_same_bits(dt):
    agg = SparsePlainAggregator(PYU("server", None))
    parties = _parties(3, dt, "overlap", seed=5)
    w = [3, 1, 2]
    all_dev = agg.average(_objs(parties, lambda k: True), axis=0, weights=w).data
    mixed = agg.average(_objs(parties, lambda k: k == 1), axis=0, weights=w).data
    host = agg.average(_objs(parties, lambda k: False), axis=0, weights=w).data
    for li, (a, m, h) in enumerate(zip(all_dev, mixed, host)):
        if LAYERS[li] == (1,):
            continue
        assert m.is_cuda and np.array_equal(_bits(_host(m)), _bits(_host(a))), li
        assert np.array_equal(_bits(_host(m)), _bits(h)), li
    # a single entry per party instead of a per-layer list, encoded on the device
    from sfl_amd import hostpipe as H

    singles = [PYUObject(PYU(f"p{k}", None), sparse_encode([H.h2d(p[0], torch.device(DEV))])[0])
               for k, p in enumerate(parties)]
    assert all(s.data.is_device for s in singles)
    got = agg.sum(singles, axis=0).data
    assert got.is_cuda and co.same_bits(_host(got), co.total([p[0] for p in parties], axis=0))
    # other axes go through numpy itself, device entries through pinned memory
    got = agg.sum(singles, axis=None).data
    assert co.same_bits(got, co.total([p[0] for p in parties], axis=None))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_overflow_and_inf_minus_inf(dt):
    """The constructed positions, and no others, are NaN, as in numpy; every
    other element is compared by bits (NaN payloads are not)."""
    agg = SparsePlainAggregator(PYU("server", None))
    big = np.finfo(dt).max
    n = 300
    rng = np.random.default_rng(3)
    xs = [np.where(rng.random(n) < 0.5, rng.standard_normal(n), 0.0).astype(dt) for _ in range(3)]
    for k, vals in enumerate(((big, np.inf, big, -np.inf), (big, -np.inf, big, 1.0), (1.0, 1.0, -big, np.inf))):
        xs[k][[7, 100, 257, 299]] = vals
    # 7: big + big overflows to inf; 100: inf - inf; 257: inf + (-big) stays inf; 299: -inf + inf
    nan_at = [100, 299]
    objs = [PYUObject(PYU(f"p{k}", None), [sparse_encode([x])[0].to(DEV)]) for k, x in enumerate(xs)]
    for call, kw in (("sum", {}), ("average", {}), ("average", {"weights": [2, 1, 1]})):
        with np.errstate(all="ignore"):
            ref = co.total(xs, axis=0) if call == "sum" else co.average(xs, axis=0, **kw)
        assert np.flatnonzero(np.isnan(ref)).tolist() == nan_at and len(nan_at) <= 8  # checked on the CPU
        got = _host(getattr(agg, call)(objs, axis=0, **kw).data[0])
        assert got.dtype == ref.dtype
        assert np.flatnonzero(np.isnan(got)).tolist() == nan_at, (call, kw)
        rest = ~np.isnan(ref)
        if not kw:
            assert np.isinf(ref[7]) and np.isinf(ref[257])  # the overflow is there (float64 sums of float32 have none)
        assert np.array_equal(_bits(got[rest]), _bits(co.plus_zero(ref)[rest])), (call, kw)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_denormal_quotient(dt):
    agg = SparsePlainAggregator(PYU("server", None))
    tiny = np.finfo(dt).tiny  # the least normal value
    xs = [np.zeros(40, dt) for _ in range(3)]
    xs[0][[0, 17, 39]] = (tiny, -tiny, 5 * tiny)
    xs[2][17] = tiny / 2  # a denormal input
    objs = [PYUObject(PYU(f"p{k}", None), [sparse_encode([x])[0].to(DEV)]) for k, x in enumerate(xs)]
    got = _host(agg.average(objs, axis=0).data[0])
    ref = co.average(xs, axis=0)
    assert 0 < ref[0] < tiny  # tiny / 3 is denormal
    assert got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(co.plus_zero(ref)))
