"""pack=2 on the GPU (two 32-bit fixed-point values per ring word) against
the numpy oracle: ``oracle.secagg.quantize`` -> ``pack_words`` ->
``mask_client`` / ``server_sum`` on the words.  Every comparison is exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gpu_copies import DEV, _dev, _host, _item, _u64  # noqa: E402
from oracle import secagg as o  # noqa: E402
from sfl_amd.security.aggregation.packing import pack_words, unpack_words  # noqa: E402

pytestmark = pytest.mark.gpu


def _inputs(C, n):
    """x_c = default_rng(c).standard_normal(n) * 1e-2 with negative and zero
    values planted at 0, n - 2 and n - 1; weights c + 1."""
    xs = []
    for c in range(C):
        x = np.random.default_rng(c).standard_normal(n, dtype=np.float32) * np.float32(1e-2)
        for pos, v in ((0, -0.25), (n - 2, -0.125), (n - 1, 0.0)):
            if pos >= 0:
                x[pos] = v
        xs.append(x)
    return xs, [c + 1 for c in range(C)]


def _pairs(names, seeds):
    from sfl_amd import _lib as L

    C = len(names)
    pg = [L.pcg64_from_seed(seeds[names[u]][names[v]]) for u in range(C) for v in range(u + 1, C)]
    return pg, [1 if names[v] > names[u] else -1 for u in range(C) for v in range(u + 1, C)]


@pytest.mark.parametrize("C, n, fxp", [(C, n, 18) for C in (2, 3, 8)
                                       for n in (1, 2, 3, 5, 1023, 1024, 1025, 2051, 9_000_011)] + [(3, 2051, 0)])
def test_fused_sum_wire_images_and_digests(C, n, fxp):
    from sfl_amd import kernels as K

    names = [f"client{c}" for c in range(C)]
    seeds = o.seeds_for(names)
    xs, ws = _inputs(C, n)
    if fxp == 0:  # values that survive truncation without a scale
        xs = [x * np.float32(1e4) for x in xs]
    words = [pack_words(o.quantize(x, w, fxp).view(np.int64), C) for x, w in zip(xs, ws)]
    masked = [o.mask_client(W, nm, seeds[nm]) for W, nm in zip(words, names)]
    S = o.server_sum(masked)
    pg, ps = _pairs(names, seeds)
    dxs, nw = [_dev(x) for x in xs], (n + 1) // 2
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    # the sum-only instance
    s = torch.empty(nw, dtype=torch.int64, device=DEV)
    K.fused_clients_pack2(dxs, ws, pg, ps, s, fxp_bits=fxp, flags=flags)
    assert np.array_equal(_u64(s), S)
    # the wire-image instance
    s2 = torch.empty(nw, dtype=torch.int64, device=DEV)
    dig = torch.zeros(C, dtype=torch.int64, device=DEV)
    mo = [torch.empty(nw, dtype=torch.int64, device=DEV) for _ in range(C)]
    K.fused_clients_pack2(dxs, ws, pg, ps, s2, fxp_bits=fxp, digests=dig, flags=flags, masked_outs=mo)
    assert np.array_equal(_u64(s2), S)
    for c in range(C):
        assert np.array_equal(_u64(mo[c]), masked[c]), c
    assert [int(v) for v in _u64(dig)] == [o.digest(m) for m in masked]
    assert _item(flags) == 0
    dec = K.decode_pack2(s, torch.empty(n, dtype=torch.float64, device=DEV), fxp_bits=fxp, divisor=float(sum(ws)))
    assert np.array_equal(_host(dec), o.decode(unpack_words(S, n).view(np.uint64), fxp, sum(ws)))


@pytest.mark.parametrize("n", [3, 1025])
@pytest.mark.parametrize("n_streams", [0, 1, 2, 16])
def test_single_client_launch(n_streams, n):
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    names = [f"p{c:02d}" for c in range(17)]
    me = names[8]  # peers on both sides: both signs
    peers = [nm for nm in names if nm != me][8 - n_streams // 2:8 - n_streams // 2 + n_streams]
    seeds = o.seeds_for(names)[me]
    (x,), _ = _inputs(1, n)
    W = pack_words(o.quantize(x, 3, 18).view(np.int64), 17)
    exp = o.mask_client(W, me, {p: seeds[p] for p in peers})
    streams = [(L.pcg64_from_seed(seeds[p]), 1 if p > me else -1, i) for i, p in enumerate(peers)]
    out = torch.empty((n + 1) // 2, dtype=torch.int64, device=DEV)
    acc = _dev(np.full((n + 1) // 2, 7, dtype=np.int64))
    dig = torch.zeros(1, dtype=torch.int64, device=DEV)
    K.mask_pack2(_dev(x), out, streams, 17, weight=3.0, sum_accum=acc, digest=dig)
    assert np.array_equal(_u64(out), exp)
    assert np.array_equal(_u64(acc), exp + np.uint64(7))
    assert int(_u64(dig)[0]) == o.digest(exp)


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 4099])
def test_decode_pack2_alone(n, misalign):
    from sfl_amd import kernels as K

    top = 2 ** 31 - 1
    sums = np.random.default_rng(n).integers(-top, top + 1, size=n, dtype=np.int64)
    # lo < 0 with hi at both extremes, lo at both extremes, zeros
    plant = [-1, top, -top, -top, -5, 0, top, -top][:n]
    sums[:len(plant)] = plant
    S = pack_words(sums)
    out = torch.empty(n + 1, dtype=torch.float64, device=DEV)[1 if misalign else 0:][:n]
    K.decode_pack2(_dev(S.view(np.int64), misalign=misalign), out, fxp_bits=18, divisor=3.0)
    assert np.array_equal(_host(out), unpack_words(S, n) / 2 ** 18 / 3.0)


def _aggregators(names, **kw):
    from sfl_amd.device import PYU
    from sfl_amd.security.aggregation import SecureAggregator

    seeds = o.seeds_for(names)
    pair = {(a, b): seeds[a][b] for a in names for b in names if a < b}
    pyus = [PYU(nm, 0) for nm in names]
    return pyus, [SecureAggregator(PYU("server", 0), pyus, seeds=pair, pack=p, **kw) for p in (1, 2)]


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("C", [3, 9])
def test_public_surface_equals_pack1(C, host):
    """sum and a weighted average of two layers: pack=2 == pack=1, bit for
    bit, through the fused launch (C = 3) and the per-party launches (9)."""
    from sfl_amd.device import reveal

    pyus, (a1, a2) = _aggregators([f"p{c}" for c in range(C)])
    layers = [[x[:5].copy(), x[5:].reshape(25, 41)] for x in _inputs(C, 5 + 1025)[0]]
    objs = [p(lambda d=d: d if host else [_dev(a).reshape(a.shape) for a in d])() for p, d in zip(pyus, layers)]
    for call in (lambda a: a.sum(objs, axis=0), lambda a: a.average(objs, axis=0, weights=list(range(1, C + 1)))):
        r1, r2 = reveal(call(a1)), reveal(call(a2))
        for l1, l2 in zip(r1, r2):
            assert type(l1) is type(l2) and l1.shape == l2.shape
            assert np.array_equal(l1 if host else _host(l1), l2 if host else _host(l2))
    assert a2._maskers["p0"].position("p1") == 2 * (3 + 513) and a1._maskers["p0"].position("p1") == 2 * 1030


@pytest.mark.parametrize("C", [2, 8])
def test_range_flag(C):
    """A value AT 2^31 / C (in the last partial tile) raises; one float32
    ulp below it passes and matches the oracle."""
    from sfl_amd.device import reveal

    n = 2051
    pyus, (_, agg) = _aggregators([f"p{c}" for c in range(C)])
    xs, _ = _inputs(C, n)
    at = np.float32(2.0 ** (31 - 18) / C)
    xs[C - 1][n - 1] = at
    with pytest.raises(OverflowError, match="fxp_bits=18"):
        agg.sum([p(lambda x=x: _dev(x))() for p, x in zip(pyus, xs)], axis=0)
    assert agg._maskers["p0"].position("p1") == 0  # the refused round moved no stream
    xs[C - 1][n - 1] = np.nextafter(at, np.float32(0))
    got = reveal(agg.sum([p(lambda x=x: _dev(x))() for p, x in zip(pyus, xs)], axis=0))
    assert np.array_equal(_host(got), o.decode(o.server_sum([o.quantize(x) for x in xs])))
    xs[0][0] = np.nan
    with pytest.raises(OverflowError):
        agg.sum([p(lambda x=x: _dev(x))() for p, x in zip(pyus, xs)], axis=0)
    assert agg._maskers["p0"].position("p1") == (n + 1) // 2  # only the accepted round did


@pytest.mark.parametrize("fused", [True, False])
def test_rejection_replay_on_words(fused):
    """The (bob, dave) stream's raw draw 300 is 0: the packed round, its wire
    images, digests and the next round equal numpy's rejection re-draw."""
    from sfl_amd.device import PYU, reveal
    from sfl_amd.security.aggregation import SecureAggregator
    from test_gpu_rejection import NAMES, _pair_states

    n, nw = 1001, 501
    pair = _pair_states(("bob", "dave"), 300)
    pyus = [PYU(nm, 0) for nm in NAMES]
    agg = SecureAggregator(PYU("server", 0), pyus, seeds=pair, fused=fused, keep_masked=True, pack=2)
    ora = o.OracleMaskers(NAMES, pair)
    for rnd in range(2):
        xs = [x + np.float32(rnd) for x in _inputs(4, n)[0]]
        got = reveal(agg.sum([p(lambda x=x: _dev(x))() for p, x in zip(pyus, xs)], axis=0))
        masked = [ora.mask(pack_words(o.quantize(x).view(np.int64), 4), nm) for x, nm in zip(xs, NAMES)]
        assert np.array_equal(_host(got), o.decode(unpack_words(o.server_sum(masked), n).view(np.uint64))), rnd
        for c in range(4):
            assert np.array_equal(_u64(agg.last_masked[0][c]), masked[c]), (rnd, c)
        assert [int(v) for v in _u64(agg.last_digests[0])] == [o.digest(m) for m in masked], rnd
    assert agg._maskers["bob"].position("dave") == 2 * nw + 1 and agg._maskers["alice"].position("bob") == 2 * nw
