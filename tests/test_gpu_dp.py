"""DP pre-step on the GPU vs the oracle (oracle/dp.py):
norm reduction, clip (exact), Philox noise (within float tolerance of the
numpy restatement), and the fused sa_mask_dp == perturb-then-mask bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from gpu_copies import DEV, _dev, _host, _item, _u64  # noqa: E402
from oracle import dp as D  # noqa: E402
from oracle import secagg as o  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _K():
    from sfl_amd import kernels as K

    return K


def _sumsq(x):
    from sfl_amd import _lib as L

    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=DEV)
    return _K().sumsq_f32(x, out, part)


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 1_000_003])
def test_sumsq_deterministic_and_accurate(n):
    """sa_sumsq_f32 = the layer's np.linalg.norm(x) ** 2 as the reference
    forms it under numpy 1.23.5 (oracle layer_sq_norm: the float32 norm
    squared in float64), deterministic; accumulating two layers adds in
    float64 (the reference's python sum)."""
    x = torch.randn(n, device=DEV)
    a, b = _sumsq(x), _sumsq(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    xh = _host(x)
    assert _item(a) == float(D.layer_sq_norm(xh))
    nrm = np.sqrt(_item(a))
    assert np.float32(nrm) == nrm and nrm * nrm == _item(a)  # the exact square of a float32 norm
    from sfl_amd import _lib as L

    part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=DEV)
    y = torch.randn(n + 5, device=DEV)
    _K().sumsq_f32(y, a, part, accumulate=True)
    assert _item(a) == float(D.global_sq([xh, _host(y)]))


# k_sumsq_partial's grid is capped at 1,024 blocks x 256 lanes x one float4:
# beyond GRID_ELEMS elements a lane takes further trips of its grid-stride
# loop, beyond 2 GRID_ELEMS the unrolled body (two loads in flight)
GRID_ELEMS = 1_048_576
SUMSQ_SIZES = [GRID_ELEMS, GRID_ELEMS + 1, 2 * GRID_ELEMS, 2 * GRID_ELEMS + GRID_ELEMS // 2 + 3,
               3 * GRID_ELEMS + 7 * 1024 + 2, 5 * GRID_ELEMS + 1]


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_multi_trip_exact(n):
    """The grid-stride loop of k_sumsq_partial (one full grid; one element
    more; the unrolled trip alone; an unrolled trip, a remainder trip for
    half the lanes and 3 tail elements; further mixes) with inputs whose
    squared norm is exact in any summation order, so a float4 that is skipped
    or read twice cannot pass:

    * all ones: the dot is exactly n < 2^24;
    * one element of 3.0 at the ends, at the last whole float4 and on either
      side of the first and second grid boundary: exactly 9.0;
    * two such elements: a dot of exactly 18 (the reference's float32 norm
      squared, 17.999999..., as D.layer_sq_norm forms it), and 3.0 with 4.0:
      exactly 25.0."""
    x = torch.ones(n, device=DEV)
    got = _item(_sumsq(x))
    assert got == float(np.float32(np.sqrt(np.float32(n)))) ** 2
    assert got == float(D.layer_sq_norm(np.ones(n, dtype=np.float32)))
    x.zero_()
    assert _item(_sumsq(x)) == 0.0
    pos = sorted({p for p in (0, 4 * (n // 4) - 1, n - 1, GRID_ELEMS - 1, GRID_ELEMS, 2 * GRID_ELEMS - 1,
                              2 * GRID_ELEMS) if 0 <= p < n})
    for p in pos:
        x[p] = 3.0
        assert _item(_sumsq(x)) == 9.0, p
        x[p] = 0.0
    two = float(np.float32(np.sqrt(np.float32(18.0)))) ** 2
    assert two == float(D.layer_sq_norm(np.array([3.0, 3.0], dtype=np.float32))) and abs(two - 18.0) < 18 * 2.0**-22
    for p, q in list(zip(pos, pos[1:])) + [(pos[0], pos[-1])]:
        x[p] = 3.0
        x[q] = 3.0
        assert _item(_sumsq(x)) == two, (p, q)
        x[q] = 4.0
        assert _item(_sumsq(x)) == 25.0, (p, q)
        x[p] = 0.0
        x[q] = 0.0


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_multi_trip_random(n):
    """The same sizes with random data: equal to the oracle's layer_sq_norm
    (the exact dot rounded once to float32), deterministic, and a second
    layer accumulates as the oracle's global_sq."""
    from sfl_amd import _lib as L

    x = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(n))
    a, b = _sumsq(x), _sumsq(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    xh = _host(x)
    assert _item(a) == float(D.layer_sq_norm(xh))
    part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=DEV)
    y = x[: 2 * GRID_ELEMS + 4 * 77 + 1] * 0.5 if n > 3 * GRID_ELEMS else x[4: n - 1] * 0.5
    assert y.data_ptr() % 16 == 0
    _K().sumsq_f32(y, a, part, accumulate=True)
    assert _item(a) == float(D.global_sq([xh, _host(y)]))


def _edge_inputs(n):
    big = np.full(n, 1e-3, dtype=np.float32)
    big[n // 3] = 1e18
    over = np.zeros(n, dtype=np.float32)
    over[5:5 + 64] = 3e18
    nan = np.linspace(-1, 1, n, dtype=np.float32)
    nan[7] = np.nan
    inf = np.linspace(-1, 1, n, dtype=np.float32)
    inf[n - 2] = np.inf
    return {"one 1e18 among 1e-3": big, "all zeros": np.zeros(n, dtype=np.float32),
            "dot above float32's range": over, "one NaN": nan, "one inf": inf}


@pytest.mark.parametrize("each_layer", [False, True])
@pytest.mark.parametrize("case", ["one 1e18 among 1e-3", "all zeros", "dot above float32's range", "one NaN",
                                  "one inf"])
def test_clip_edges_vs_oracle(case, each_layer):
    """The norm, the clip scale and the perturbed output at inputs where the
    float32 norm saturates, vanishes or is not a number, against oracle/dp.py
    with the same inputs (n = 4099): a zero norm leaves the scale at 1 (the
    input comes back bit for bit without noise, and exactly the noise with
    it); a dot above float32's range makes the norm inf and the scale 0; a
    NaN norm fails ``r < 1`` and leaves the scale at 1.  With each_layer the
    total is this layer's square plus another layer's."""
    K = _K()
    from sfl_amd import _lib as L

    n, clip, key, ctr = 4099, 0.5, 0xC0FFEE, 4 * 9
    xh = _edge_inputs(n)[case]
    x = _dev(xh)
    with np.errstate(all="ignore"):
        want_sq = D.layer_sq_norm(xh)
    layer = _sumsq(x)
    assert np.array_equal(_host(layer), np.array([want_sq]), equal_nan=True), (_item(layer), want_sq)
    if case == "all zeros":
        assert _item(layer) == 0.0
    elif case in ("dot above float32's range", "one inf"):
        assert _item(layer) == np.inf
    elif case == "one NaN":
        assert np.isnan(_item(layer))
    else:
        assert abs(_item(layer) / 1e36 - 1) < 1e-6  # finite: float32 holds the dot, float64 the partial sums
    total, other = layer, np.full(100, 1.5, dtype=np.float32)
    if each_layer:
        total = layer.clone()
        part = torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=DEV)
        K.sumsq_f32(_dev(other), total, part, accumulate=True)
        with np.errstate(all="ignore"):
            want_total = D.global_sq([xh, other])
        assert np.array_equal(_host(total), np.array([want_total]), equal_nan=True)
    with np.errstate(all="ignore"):
        scale = D.clip_scale(_item(total), clip, _item(layer) if each_layer else None)
    assert scale == {"one 1e18 among 1e-3": scale, "all zeros": 1.0, "dot above float32's range": 0.0, "one NaN": 1.0,
                     "one inf": 0.0}[case]
    assert 0.0 <= scale <= 1.0
    kw = dict(l2_norm_clip=clip, key=key, counter0=ctr, sumsq_layer=layer if each_layer else None)
    # without noise: x * scale exactly
    y0 = _host(K.dp_perturb(x, torch.empty_like(x), K.make_dp(total, noise_std=0.0, num_updates=4, **kw)))
    with np.errstate(all="ignore"):
        exp0 = D.perturb(xh, scale, np.zeros(n, np.float32), 0.0, 4)
    assert np.array_equal(y0, exp0, equal_nan=True)
    if case == "all zeros":
        assert np.array_equal(y0.view(np.uint32), xh.view(np.uint32))
    # with noise
    for updates in (4, 3):
        y = K.dp_perturb(x, torch.empty_like(x), K.make_dp(total, noise_std=0.3, num_updates=updates, **kw))
        y = _host(y)
        with np.errstate(all="ignore"):
            exp = D.perturb(xh, scale, D.gauss(key, ctr, n), 0.3, updates)
        assert np.allclose(y, exp, rtol=2e-5, atol=2e-6, equal_nan=True)
        assert np.array_equal(np.isnan(y), np.isnan(exp))
        if case == "all zeros":  # exactly the noise: what a zero input gives under any other norm
            s1 = _sumsq(torch.ones(4, device=DEV))
            z = K.dp_perturb(x, torch.empty_like(x), K.make_dp(s1, l2_norm_clip=clip, noise_std=0.3,
                                                                num_updates=updates, key=key, counter0=ctr))
            assert np.array_equal(y.view(np.uint32), _host(z).view(np.uint32))
            # the normal's tolerance scaled by sigma / updates, plus the two float32 roundings
            f = np.float64(np.float32(0.3)) / updates
            z64 = D.gauss64(key, ctr, n)
            assert np.all(np.abs(y - f * z64) <= f * (2e-5 * np.abs(z64) + 2e-6) + 2.0**-22 * f * np.abs(z64))


@pytest.mark.parametrize("clip", [0.5, 1e6])
def test_perturb_clip_exact_without_noise(clip):
    K = _K()
    n = 70_001
    x = torch.randn(n, device=DEV) * 3
    s = _sumsq(x)
    dp = K.make_dp(s, l2_norm_clip=clip, noise_std=0.0, num_updates=4, key=1)
    y = K.dp_perturb(x, torch.empty_like(x), dp)
    torch.cuda.synchronize()
    scale = D.clip_scale(_item(s), clip)
    assert np.array_equal(_host(y), _host(x) * scale)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 262_147])
def test_perturb_tile_edges_and_no_write_past_n(n):
    """The tile form's whole-tile and partial-tile paths (1,024 elements per
    workgroup) against the oracle's noise stream; the 16 floats after n keep
    their sentinel."""
    K = _K()
    key, ctr = 0x0123456789ABCDEF, 4 * 7
    x = torch.randn(n, device=DEV) * 0.2
    s = _sumsq(x)
    buf = torch.full((n + 16,), 12345.0, device=DEV)
    dp = K.make_dp(s, l2_norm_clip=0.5, noise_std=0.3, num_updates=4, key=key, counter0=ctr)
    K.dp_perturb(x, buf[:n], dp)
    torch.cuda.synchronize()
    assert torch.all(buf[n:] == 12345.0)
    xh = _host(x)
    exp = D.perturb(xh, D.clip_scale(_item(s), 0.5), D.gauss(key, ctr, n), 0.3, 4)
    assert np.allclose(_host(buf[:n]), exp, rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("updates", [4, 3])
def test_perturb_noise_matches_oracle_stream(updates):
    K = _K()
    n, key, ctr = 100_003, 0xDEADBEEF12345678, 4 * 1000
    x = torch.zeros(n, device=DEV)
    s = _sumsq(torch.ones(4, device=DEV))
    dp = K.make_dp(s, l2_norm_clip=1.0, noise_std=1.5, num_updates=updates, key=key, counter0=ctr)
    y = _host(K.dp_perturb(x, torch.empty_like(x), dp))
    z = D.gauss(key, ctr, n)
    exp = D.perturb(np.zeros(n, np.float32), 1.0, z, 1.5, updates)
    assert np.allclose(y, exp, rtol=2e-5, atol=2e-6)
    assert abs(y.mean()) < 0.01 and abs(y.std() - 1.5 / updates) < 0.01


@pytest.mark.parametrize("nstreams,updates", [(0, 8), (3, 8), (17, 8), (3, 3), (7, 6)])
def test_fused_mask_dp_equals_perturb_then_mask(nstreams, updates):
    K, L = _K(), None
    from sfl_amd import _lib as L

    n = 50_003
    x = torch.randn(n, device=DEV) * 0.05
    s = _sumsq(x)
    seeds = [o.pair_seed(0, j + 1) for j in range(nstreams)]
    streams = [(L.pcg64_from_seed(sd), 1 if j % 2 else -1, j) for j, sd in enumerate(seeds)]
    # num_updates a power of two: the kernels multiply by the exact reciprocal; else IEEE division
    mk = lambda: K.make_dp(s, l2_norm_clip=0.3, noise_std=0.01, num_updates=updates, key=77, counter0=40)  # noqa: E731
    xp = K.dp_perturb(x, torch.empty_like(x), mk())
    m1 = torch.empty(n, dtype=torch.int64, device=DEV)
    d1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    K.mask(xp, m1, streams, weight=3.0, digest=d1)
    m2 = torch.empty(n, dtype=torch.int64, device=DEV)
    d2 = torch.zeros(1, dtype=torch.int64, device=DEV)
    K.mask_dp(x, m2, streams, mk(), weight=3.0, digest=d2)
    torch.cuda.synchronize()
    bad = (m1 != m2).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} masked elements differ, first {_host(bad[:8]).tolist()}"
    assert torch.equal(d1, d2)
    # and the masked vector is the oracle's for the perturbed input
    exp = o.quantize(_host(xp), 3)
    for sd, (_, sg, _) in zip(seeds, streams):
        mm = o.mask_stream(sd, n)
        exp = exp + mm if sg > 0 else exp - mm
    assert np.array_equal(_u64(m2), exp)


@pytest.mark.parametrize("each_layer", [False, True])
def test_gaussian_model_dp_class_vs_oracle(each_layer):
    from sfl_amd.security.privacy import GaussianModelDP

    rng = np.random.default_rng(5)
    layers = [rng.standard_normal((50, 4)).astype(np.float32), rng.standard_normal(50).astype(np.float32),
              rng.standard_normal((3, 50)).astype(np.float32)]
    dp = GaussianModelDP(noise_multiplier=0.7, num_clients=8, l2_norm_clip=2.0, is_clip_each_layer=each_layer,
                         seed=99)
    got = dp(layers)
    exp = D.gaussian_model_dp(layers, 0.7, 8, 2.0, key=99, is_clip_each_layer=each_layer)
    for g, e, a in zip(got, exp, layers):
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == a.shape
        assert np.allclose(g, e, rtol=1e-5, atol=1e-6)
    # noise-free: exact clip
    dp0 = GaussianModelDP(noise_multiplier=0.0, num_clients=8, l2_norm_clip=2.0, seed=1)
    got0 = dp0(layers)
    exp0 = D.gaussian_model_dp(layers, 0.0, 8, 2.0)
    for g, e in zip(got0, exp0):
        assert np.array_equal(g, e)


@pytest.mark.parametrize("each_layer", [False, True])
def test_gaussian_model_dp_called_twice_advances_the_noise(each_layer):
    """The same instance on the same layers twice (sizes that are no multiple
    of 4, a zero-size layer, a 2-d layer): the second call's noise is the
    stream from counter sum(ceil4(size)) on -- the oracle's with that
    counter0 -- and differs from the first call's in every non-empty layer
    (two rounds sharing their noise would let the server subtract it);
    torch tensors in and out give the same values as numpy in and out."""
    from sfl_amd.security.privacy import GaussianModelDP

    rng = np.random.default_rng(11)
    shapes = [(1,), (3,), (5,), (7, 9), (0,), (4096,)]
    layers = [(rng.standard_normal(s) * 0.3).astype(np.float32) for s in shapes]
    step = sum(-(-a.size // 4) * 4 for a in layers)
    assert step == 4 + 4 + 8 + 64 + 0 + 4096
    mk = lambda: GaussianModelDP(noise_multiplier=0.7, num_clients=8, l2_norm_clip=2.0,  # noqa: E731
                                 is_clip_each_layer=each_layer, seed=99)
    dp = mk()
    calls = [dp(layers), dp(layers)]
    assert dp.counter == 2 * step
    for c, got in enumerate(calls):
        exp = D.gaussian_model_dp(layers, 0.7, 8, 2.0, key=99, counter0=c * step, is_clip_each_layer=each_layer)
        for g, e, a in zip(got, exp, layers):
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == a.shape
            assert np.allclose(g, e, rtol=2e-5, atol=2e-6), (c, a.shape)
    for g1, g2 in zip(*calls):
        if g1.size:
            assert np.mean(g1 != g2) > 0.99 and g1.reshape(-1)[0] != g2.reshape(-1)[0]
    dpt = mk()
    tin = [_dev(a).reshape(a.shape) for a in layers]
    for got in calls:
        tout = dpt(tin)
        for t, g in zip(tout, got):
            assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == g.shape
            assert np.array_equal(_host(t).view(np.uint32), g.view(np.uint32))
    assert dpt.counter == 2 * step
    for t, a in zip(tin, layers):  # the inputs are left alone
        assert np.array_equal(_host(t), a)


def _reference_clip_numpy(inputs, clip, each_layer):
    """mechanism_fl.py:71-108 with noise_multiplier = 0, restated on numpy's
    own float32 arithmetic (np.linalg.norm per layer, ** 2, python sum,
    np.sqrt, min(1, clip / norm), the float32 array times the scale).  Runs
    under this image's numpy 2 (NEP 50: clip / float32 divides in float32,
    where the reference's numpy 1.23.5 divides in float64 -- within one ulp
    of the scale)."""
    def gnorm(arrs):
        return np.sqrt(sum([np.linalg.norm(a) ** 2 for a in arrs]))

    norm_all = gnorm(inputs)
    if each_layer:
        return [a * min(1, clip / np.sqrt(gnorm([a]) * norm_all)) for a in inputs]
    scale = min(1, clip / norm_all)
    return [a * scale for a in inputs]


@pytest.mark.parametrize("each_layer", [False, True])
@pytest.mark.parametrize("clip", [0.5, 1e6])
def test_gaussian_model_dp_vs_reference_numpy_clip(each_layer, clip):
    """GaussianModelDP with noise_multiplier = 0 against
    the reference's clip evaluated by numpy itself.  The device forms the
    norm with the reference's float32 structure (sa_sumsq_f32); what is left
    is the reference's BLAS float32 dot, whose accumulation error the test
    measures (|np.linalg.norm - exact| / exact) and allows, plus 4 ulps of
    float32 for the scale's division and the product.  With no clipping
    (clip 1e6: scale 1) the output is the input bit for bit."""
    from sfl_amd.security.privacy import GaussianModelDP

    rng = np.random.default_rng(17)
    layers = [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in ((300, 200), (200,), (200, 10), (10,))]
    layers.append((rng.standard_normal(1_000_003) * 0.01).astype(np.float32))
    dp = GaussianModelDP(noise_multiplier=0.0, num_clients=8, l2_norm_clip=clip, is_clip_each_layer=each_layer,
                         seed=3)
    got = dp(layers)
    ref = _reference_clip_numpy(layers, clip, each_layer)
    exact = [np.sqrt(np.sum(a.astype(np.float64) ** 2)) for a in layers]
    blas_rel = max(abs(float(np.linalg.norm(a)) - e) / e for a, e in zip(layers, exact))
    tot_exact = np.sqrt(sum(e * e for e in exact))
    blas_rel = max(blas_rel, abs(float(np.sqrt(sum([np.linalg.norm(a) ** 2 for a in layers]))) - tot_exact) / tot_exact)
    tol = 2 * blas_rel + 4 * 2.0**-24
    for g, r, a in zip(got, ref, layers):
        assert g.dtype == np.float32 and r.dtype == np.float32
        if clip == 1e6:
            assert np.array_equal(g, a) and np.array_equal(r, a)
        else:
            np.testing.assert_allclose(g, r, rtol=tol, atol=0)


def test_loopback_client_dp_round_vs_oracle():
    """LoopbackClient.submit(dp=...) with in-process parties over 127.0.0.1:
    every client perturbs its device copy (GaussianModelDP: clip to the
    global norm + Philox noise) and masks it; the server's decoded sum equals
    the oracle's sum of the perturbed vectors bit for bit (the noise taken
    from the standalone perturb kernel, which test_fused_mask_dp_equals_
    perturb_then_mask pins to the fused kernel).  Two rounds with the same
    clients and the same GaussianModelDP instances: round 2's noise is the
    next window of each client's stream (a second params call on the
    expected side), never round 1's again -- the server could subtract two
    rounds that share their noise."""
    import threading

    from sfl_amd.loopback import LoopbackClient, LoopbackServer
    from sfl_amd.security.privacy import GaussianModelDP

    K = _K()
    names, n, rounds = ["p0", "p1", "p2"], 30_011, 2
    seeds = o.seeds_for(names)
    rng = np.random.default_rng(9)
    xs = [(rng.standard_normal(n) * 0.05).astype(np.float32) for _ in names]
    srv = LoopbackServer(len(names))
    res = {}

    def client(i):
        cl = LoopbackClient(names[i], i, srv.port, seeds={v: seeds[names[i]][v] for v in names if v != names[i]})
        cl.handshake()
        dp = GaussianModelDP(noise_multiplier=0.5, num_clients=3, l2_norm_clip=0.8, seed=100 + i)
        for r in range(rounds):
            out = np.empty(n, dtype=np.float64)
            cl.submit(xs[i], r, dp=dp, result_into=out)
            res[i, r] = (cl.result(n), cl.last_result_xor)
        res[i, "counter"] = dp.counter
        cl.close()

    ts = [threading.Thread(target=client, args=(i,)) for i in range(len(names))]
    for t in ts:
        t.start()
    srv.accept(timeout=60)
    got = [np.array(srv.round(n, r)[0]) for r in range(rounds)]
    for t in ts:
        t.join(60)
    srv.close()
    # the expected perturbed inputs, from the same DP parameters: one instance
    # per client, params called once per round
    dps = [GaussianModelDP(noise_multiplier=0.5, num_clients=3, l2_norm_clip=0.8, seed=100 + i)
           for i in range(len(names))]
    exps, xps = [], []
    for r in range(rounds):
        xp = []
        for dp, x in zip(dps, xs):
            d = _dev(x)
            xp.append(_host(K.dp_perturb(d, torch.empty_like(d), dp.params(dp.sumsq([d]), n))))
        exp = o.secure_sum(xp, names, seeds=seeds, offset=r * n)[0]
        assert np.array_equal(got[r], exp), r
        for i in range(len(names)):
            assert np.array_equal(res[i, r][0], exp)
            assert res[i, r][1] == int(np.bitwise_xor.reduce(exp.view(np.uint64)))
        assert float(np.abs(exp - np.sum(xs, axis=0)).max()) > 1e-4  # the noise is there
        exps.append(exp)
        xps.append(xp)
    n4 = -(-n // 4) * 4
    for i, dp in enumerate(dps):
        assert dp.counter == rounds * n4 and res[i, "counter"] == rounds * n4
        # round 2's noise is the stream's next window, not round 1's (the inputs are the same)
        assert np.mean(xps[0][i] != xps[1][i]) > 0.99
        z2 = D.gauss(100 + i, n4, n)
        exp2 = D.perturb(xs[i], D.clip_scale(_item(dp.sumsq([_dev(xs[i])])), 0.8), z2,
                         0.5 * 0.8 * 0.8, 3)
        assert np.allclose(xps[1][i], exp2, rtol=2e-5, atol=2e-6)
    assert np.mean(exps[0] != exps[1]) > 0.99
