"""FedSMP on the GPU: the sa_smp kernels against the host mask and the numpy
chain (tests/smp_oracle.py), the fused pass against the unfused three, the
three forms of smp_step against each other, and FLModel("fed_smp") with a GPU
model through the secure aggregator against the CPU run."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

import smp_oracle as so  # noqa: E402
from gpu_copies import DEV, _dev, _host, _item  # noqa: E402
from oracle import dp as D  # noqa: E402
from oracle import secagg as o  # noqa: E402

pytestmark = pytest.mark.gpu

KEY, DPKEY = 0x0123456789ABCDEF, 0x5EED5EED5EED5EED
# the tile kernels take 4 elements per lane and 256 lanes per block; the sumsq grid holds
# 1,024 blocks, so above 1,048,576 elements a lane takes a second trip
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 3 - 1, 4 * 256 * 3 + 1, 1_048_576 + 1_029]
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _K():
    from sfl_amd import kernels as K

    return K


_CACHE = {}


def _pair(n):
    """(w0, w1) of n elements on the host, made once per size and left unchanged."""
    if n not in _CACHE:
        rng = np.random.default_rng(n)
        w0 = rng.standard_normal(n).astype(np.float32)
        _CACHE[n] = (w0, w0 + (rng.standard_normal(n) * 0.05).astype(np.float32))
    return _CACHE[n]


def _smp(p, counter0):
    K = _K()
    return K.make_smp(KEY, counter0, so.threshold(p), float(so.divisor(p)))


def _delta(w0, w1, p, counter0):
    with np.errstate(all="ignore"):
        return np.where(so.kept(KEY, p, counter0, w0.size), (w1 - w0) / so.divisor(p), np.float32(0))


def _guarded(n, dtype=torch.float32):
    """An output of n elements with GUARD sentinel elements behind it."""
    buf = torch.full((n + GUARD,), 77, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _guard_intact(buf, n):
    return bool((buf[n:] == 77).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sumsq_scratch():
    from sfl_amd import _lib as L

    return torch.empty(L.SA_DP_PARTIALS, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("n", SIZES)
def test_mask_on_the_device_equals_the_host(n):
    from sfl_amd import _lib as L

    K = _K()
    for p, counter0 in ((0.5, 0), (0.1, 4096), (1.0, 8), (0.0, 8)):
        smp = _smp(p, counter0)
        buf, out = _guarded(n, torch.uint8)
        K.smp_mask(smp, out)
        want = L.smp_mask_host(smp, n)
        assert np.array_equal(_host(out), want) and _guard_intact(buf, n)
        assert np.array_equal(want.astype(bool), so.kept(KEY, p, counter0, n))
    if n:  # an output that is only byte-aligned
        buf = torch.full((n + 1 + GUARD,), 77, dtype=torch.uint8, device=DEV)
        K.smp_mask(_smp(0.5, 4), buf[1:n + 1])
        assert np.array_equal(_host(buf[1:n + 1]), L.smp_mask_host(_smp(0.5, 4), n))
        assert _item(buf[0]) == 77 and _guard_intact(buf, n + 1)


@pytest.mark.parametrize("n", SIZES)
def test_delta_and_its_norm(n):
    """sa_smp_delta_f32 is the numpy d in bits; sa_smp_sumsq_f32 is sa_sumsq_f32 of it in bits, with
    accumulate on and off."""
    K = _K()
    w0h, w1h = _pair(n)
    w0, w1 = _dev(w0h), _dev(w1h)
    part = _sumsq_scratch()
    for p, counter0 in ((0.5, 0), (0.1, 4096), (0.8, 2**34 + 4), (1.0, 0), (0.0, 0)):
        smp = _smp(p, counter0)
        buf, d = _guarded(n)
        K.smp_delta(w0, w1, smp, d)
        assert np.array_equal(_bits(_host(d)), _bits(_delta(w0h, w1h, p, counter0))) and _guard_intact(buf, n)
        want = K.sumsq_f32(d, torch.zeros(1, dtype=torch.float64, device=DEV), part)
        got = K.smp_sumsq(w0, w1, smp, torch.full((1,), 5.0, dtype=torch.float64, device=DEV), part)
        assert _item(got) == _item(want) == float(D.layer_sq_norm(_host(d)))
        acc_want = K.sumsq_f32(d, torch.full((1,), 0.375, dtype=torch.float64, device=DEV), part, accumulate=True)
        acc_got = K.smp_sumsq(w0, w1, smp, torch.full((1,), 0.375, dtype=torch.float64, device=DEV), part,
                              accumulate=True)
        assert _item(acc_got) == _item(acc_want)


def _norms(K, w0, w1, smp, each_layer, extra=0.25):
    """(total, layer): the total holds another layer's square already."""
    part = _sumsq_scratch()
    total = K.smp_sumsq(w0, w1, smp, torch.full((1,), extra, dtype=torch.float64, device=DEV), part, accumulate=True)
    layer = K.smp_sumsq(w0, w1, smp, torch.zeros(1, dtype=torch.float64, device=DEV), part) if each_layer else None
    return total, layer


@pytest.mark.parametrize("each_layer", [False, True], ids=["global", "each_layer"])
@pytest.mark.parametrize("updates", [4, 3], ids=["pow2", "div"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_equals_unfused_with_noise(n, updates, each_layer):
    K = _K()
    w0h, w1h = _pair(n)
    w0, w1 = _dev(w0h), _dev(w1h)
    for p, c_smp, c_dp in ((0.5, 4096, 8), (0.1, 0, 0)):
        smp = _smp(p, c_smp)
        total, layer = _norms(K, w0, w1, smp, each_layer)
        dp = K.make_dp(total, l2_norm_clip=0.5, noise_std=0.3, num_updates=updates, key=DPKEY, counter0=c_dp,
                       sumsq_layer=layer)
        buf, fused = _guarded(n)
        K.smp_perturb(w0, w1, smp, dp, fused)
        d = K.smp_delta(w0, w1, smp, torch.empty_like(w0))
        t = K.dp_perturb(d, torch.empty_like(d), dp)
        buf2, unfused = _guarded(n)
        K.smp_finish(w0, t, smp, unfused)
        got, want = _host(fused), _host(unfused)
        assert np.array_equal(_bits(got), _bits(want)) and _guard_intact(buf, n) and _guard_intact(buf2, n)
        kept = so.kept(KEY, p, c_smp, n)
        assert np.array_equal(_bits(got)[~kept], _bits(w0h)[~kept])
        if n >= 1023:
            assert not np.array_equal(got[kept], w0h[kept])
        # out may be w1
        alias = w1.clone()
        K.smp_perturb(w0, alias, smp, dp, alias)
        assert np.array_equal(_bits(_host(alias)), _bits(want))


@pytest.mark.parametrize("each_layer", [False, True], ids=["global", "each_layer"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_without_noise_is_the_host_form(n, each_layer):
    """sigma = 0: the by-hand float32 chain with oracle.dp's clip, bit for bit; without a dp,
    kept ? w0 + d : w0."""
    K = _K()
    w0h, w1h = _pair(n)
    w0, w1 = _dev(w0h), _dev(w1h)
    for p, c_smp, updates in ((0.5, 4096, 4), (0.8, 0, 3)):
        smp = _smp(p, c_smp)
        kept = so.kept(KEY, p, c_smp, n)
        dh = _delta(w0h, w1h, p, c_smp)
        plain = _host(K.smp_perturb(w0, w1, smp, None, torch.empty_like(w0)))
        assert np.array_equal(_bits(plain), _bits(np.where(kept, w0h + dh, w0h)))
        total, layer = _norms(K, w0, w1, smp, each_layer, extra=0.0)
        assert _item(total) == float(D.layer_sq_norm(dh))
        for clip in (0.5, 1e6):
            dp = K.make_dp(total, l2_norm_clip=clip, noise_std=0.0, num_updates=updates, key=DPKEY, counter0=12,
                           sumsq_layer=layer)
            got = _host(K.smp_perturb(w0, w1, smp, dp, torch.empty_like(w0)))
            scale = D.clip_scale(D.layer_sq_norm(dh), clip, D.layer_sq_norm(dh) if each_layer else None)
            t = D.perturb(dh, scale, D.gauss(DPKEY, 12, n), 0.0, updates)
            assert np.array_equal(_bits(got), _bits(np.where(kept, w0h + t, w0h))), (p, clip)


@pytest.mark.parametrize("updates", [4, 3], ids=["pow2", "div"])
@pytest.mark.parametrize("n", [5, 1025, 4 * 256 * 3 + 1])
def test_fused_noise_against_the_oracle_normals(n, updates):
    """tests/test_gpu_dp.py's noise tolerance (the device's Box-Muller against numpy's: rtol 2e-5,
    atol 2e-6 on a normal) scaled by sigma / num_updates, plus the four float32 roundings that
    follow the normal (z sigma, / num_updates, + d scale, + w0), each at most 2^-24 of the
    magnitudes involved."""
    K = _K()
    w0h, w1h = _pair(n)
    w0, w1 = _dev(w0h), _dev(w1h)
    p, c_smp, c_dp, sigma = 0.5, 8, 4096, 0.3
    smp = _smp(p, c_smp)
    total, _ = _norms(K, w0, w1, smp, False, extra=0.0)
    dp = K.make_dp(total, l2_norm_clip=0.5, noise_std=sigma, num_updates=updates, key=DPKEY, counter0=c_dp)
    got = _host(K.smp_perturb(w0, w1, smp, dp, torch.empty_like(w0))).astype(np.float64)
    kept = so.kept(KEY, p, c_smp, n)
    dh = _delta(w0h, w1h, p, c_smp)
    ds = (dh * D.clip_scale(D.layer_sq_norm(dh), 0.5)).astype(np.float64)
    f = np.float64(np.float32(sigma)) / updates
    z = D.gauss64(DPKEY, c_dp, n)
    want = w0h.astype(np.float64) + ds + f * z
    bound = f * (2e-5 * np.abs(z) + 2e-6) + 2.0**-22 * (np.abs(w0h) + np.abs(ds) + f * np.abs(z))
    assert np.all(np.abs(got - want)[kept] <= bound[kept])
    assert np.array_equal(got[~kept], w0h[~kept].astype(np.float64))
    assert np.abs(got - w0h - ds)[kept].max() > 0.01  # the noise is there


# --- smp_step on lists of CUDA tensors ---------------------------------------

def _lists():
    """float32 (64 x 33), int64, an empty layer, float32 (50), and a float32 layer whose device
    copy is only element-aligned."""
    rng = np.random.default_rng(21)
    old = [rng.standard_normal((64, 33)).astype(np.float32), np.array([3, 4], dtype=np.int64),
           np.zeros((0, 7), dtype=np.float32), rng.standard_normal(50).astype(np.float32),
           rng.standard_normal(1029).astype(np.float32)]
    new = [a + (rng.standard_normal(a.shape) * 0.05).astype(np.float32) if a.dtype == np.float32 else a + 1 for a in old]
    return old, new


def _to_dev(layers):
    return [_dev(a, misalign=(i == 4)).reshape(a.shape) for i, a in enumerate(layers)]


def _gdp(sigma_mult, each_layer=False, updates=4, seed=77):
    from sfl_amd.security.privacy import GaussianModelDP

    return GaussianModelDP(noise_multiplier=sigma_mult, num_clients=2, num_updates=updates, l2_norm_clip=0.5,
                           is_clip_each_layer=each_layer, device=DEV, seed=seed)


def _same_lists(a, b):
    for x, y in zip(a, b):
        x = _host(x) if isinstance(x, torch.Tensor) else x
        y = _host(y) if isinstance(y, torch.Tensor) else y
        if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            return False
    return True


@pytest.mark.parametrize("each_layer", [False, True], ids=["global", "each_layer"])
@pytest.mark.parametrize("updates", [4, 3], ids=["pow2", "div"])
def test_smp_step_three_forms(each_layer, updates):
    from sfl_amd.security.privacy import SMPMask, smp_step

    old, new = _lists()
    dold, dnew = _to_dev(old), _to_dev(new)
    assert dold[4].data_ptr() % 16 and dnew[4].data_ptr() % 16
    mask = SMPMask(KEY, 0.5)
    n_float = [a.size for a in old if a.dtype == np.float32]
    end = sum(-(-n // 4) * 4 for n in n_float)
    for sigma_mult in (0.0, 1.2):
        gdps = [_gdp(sigma_mult, each_layer, updates) for _ in range(3)]
        fused = smp_step(dold, dnew, mask, gdps[0])
        unfused = smp_step(dold, dnew, mask, lambda xs: gdps[1](xs))  # a callable of the user's: the unfused path
        host = smp_step(old, new, mask, gdps[2])
        assert all(t.is_cuda and t.dtype == torch.float32 for i, t in enumerate(fused) if i != 1)
        assert fused[1] is dnew[1] and host[1] is new[1]
        assert [tuple(t.shape) for t in fused] == [a.shape for a in old]
        assert _same_lists(fused, unfused) and _same_lists(unfused, host)
        assert [g.counter for g in gdps] == [end] * 3  # where __call__ leaves it
        if sigma_mult == 0.0:
            want = so.step(old, new, KEY, 0.5, so.clip_only(0.5, each_layer, updates))
            assert _same_lists(fused, want)
    # no model_gdp at all
    assert _same_lists(smp_step(dold, dnew, mask), so.step(old, new, KEY, 0.5))


def test_smp_step_with_the_secure_generator_takes_the_unfused_path():
    from sfl_amd import kernels as K
    from sfl_amd.security.privacy import SecureGaussianModelDP, SMPMask, smp_step

    old, new = _lists()
    dold, dnew = _to_dev(old), _to_dev(new)
    mask = SMPMask(KEY, 0.5)
    mk = lambda: SecureGaussianModelDP(noise_multiplier=1.2, num_clients=2, num_updates=4, l2_norm_clip=0.5,  # noqa: E731
                                       device=DEV, key=bytes(range(32)), nonce=5)
    gdp = mk()
    got = smp_step(dold, dnew, mask, gdp)
    f = [i for i, a in enumerate(old) if a.dtype == np.float32]
    # by hand: delta, the same generator on the list of d, finish
    counters = [c for c in so.counters(old) if c is not None]
    flat = [(dold[i].reshape(-1).clone(), dnew[i].reshape(-1).clone()) for i in f]
    ds = [K.smp_delta(a, b, mask.layer(c0), torch.empty_like(a)) if a.numel() else a for (a, b), c0 in zip(flat, counters)]
    ts = mk()(ds)
    for i, (a, _), t, c0 in zip(f, flat, ts, counters):
        want = K.smp_finish(a, t, mask.layer(c0), torch.empty_like(a)) if a.numel() else a
        assert np.array_equal(_bits(_host(got[i]).reshape(-1)), _bits(_host(want)))
    assert gdp.counter == sum(-(-old[i].size // 4) * 4 for i in f)
    kept = so.masks(KEY, 0.5, old)
    assert all(np.array_equal(_bits(_host(got[i]))[~kept[i]], _bits(old[i])[~kept[i]]) for i in f)


# --- FLModel ---------------------------------------------------------------------

NAMES = ["client0", "client1"]


class OnDevice:
    """An aggregator that notes where its inputs live."""

    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def average(self, data, axis=0, weights=None):
        self.seen.append(all(isinstance(t, torch.Tensor) and t.is_cuda for d in data for t in d.data))
        return self.inner.average(data, axis=axis, weights=weights)


def test_fl_model_with_a_gpu_model_and_the_secure_aggregator():
    """Two parties, two rounds, sigma = 0 (the clip stays): the aggregates of the GPU run through
    the secure aggregator against the CPU run through the oracle aggregator, within the tolerance
    the FL tests state for a float32 model against the aggregator's fixed-point result
    (tests/test_fl_stc.py: rtol 0, atol 1e-5; the grid is 2^-18).  Local training is plain SGD: it
    runs on the GPU in one run and on the CPU in the other."""
    from torch import optim

    from sfl_amd.device import PYU
    from sfl_amd.ml.fl import FLModel, TorchModel, optim_wrapper
    from sfl_amd.security.aggregation import SecureAggregator
    from sfl_amd.security.privacy import DPStrategyFL
    from test_fl_round import MlpNet, OracleAggregator, _data

    seeds = o.seeds_for(NAMES)
    pair = {(a, b): seeds[a][b] for a in NAMES for b in NAMES if a != b}
    pyus = [PYU(n, 0) for n in NAMES]
    xs, ys = _data(n_per=64)

    def run(agg, train_device):
        model = TorchModel(model_fn=MlpNet, loss_fn=nn.CrossEntropyLoss, optim_fn=optim_wrapper(optim.SGD, lr=0.05))
        fl = FLModel(server=None, device_list=pyus, model=model, aggregator=agg, strategy="fed_smp", random_seed=1234,
                     train_device=train_device, compression_ratio=0.5, dp_strategy=DPStrategyFL(_gdp(0.0)))
        rounds = []
        hist = fl.fit(dict(zip(pyus, xs[:2])), dict(zip(pyus, ys[:2])), batch_size=32, epochs=1,
                      round_hook=lambda r, a: rounds.append([_host(t) if isinstance(t, torch.Tensor) else np.asarray(t)
                                                             for t in a]))
        return fl, hist, rounds

    dev_agg = OnDevice(SecureAggregator(PYU("server", 0), pyus, seeds=pair))
    fl_dev, hist, dev_rounds = run(dev_agg, None)
    _, _, ref_rounds = run(OracleAggregator(NAMES, seeds), "cpu")
    assert dev_agg.seen == [False, True, True]  # get_weights for the initial average, then device payloads
    assert hist["mask_bytes"] == [32, 32] and len(dev_rounds) == len(ref_rounds) == 3
    assert len(fl_dev.masks) == 3
    worst = 0.0
    for a, b in zip(dev_rounds, ref_rounds):
        for x, y in zip(a, b):
            worst = max(worst, float(np.abs(x - y).max()))
            assert np.allclose(x, y, rtol=0, atol=1e-5)
    print("largest difference of an aggregate", worst)
    assert all(np.array_equal(x, y) for x, y in zip(dev_rounds[0], ref_rounds[0]))  # the initial average: bit for bit
    moved = max(float(np.abs(x - y).max()) for x, y in zip(dev_rounds[0], dev_rounds[-1]))
    assert moved > 1e-3  # training did something
