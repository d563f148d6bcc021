"""The ``fed_stc`` strategy (sparse ternary compression upstream and
downstream) on the MLP, data and helpers of test_fl_round.py.

CPU: the worker's contract (payload, residual, the discarded local step)
and a full ``fit`` with the oracle aggregator.  GPU: device compression is
deterministic, so a run through the HIP ``SecureAggregator`` equals one
through the oracle aggregator bit for bit; and device compression agrees
with the numpy path on the first round's uploads."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

from gpu_copies import _host  # noqa: E402
from oracle import secagg as o  # noqa: E402
from test_fl_round import NAMES, MlpNet, OracleAggregator, _data  # noqa: E402

LR, EPOCHS = 5e-3, 4  # test inputs, picked on the CPU so that the loss falls at sparsity 0.5


class Recording:
    """An aggregator that keeps what went into and came out of ``average``."""

    def __init__(self, inner):
        self.inner, self.uploads, self.aggregates = inner, [], []

    def average(self, data, axis=0, weights=None):
        self.uploads.append([[np.array(x, copy=True) for x in d.data] for d in data])
        out = self.inner.average(data, axis=axis, weights=weights)
        self.aggregates.append([np.array(x, copy=True) for x in out.data])
        return out


def _model(lr=LR):
    from torch import optim

    from sfl_amd.ml.fl import TorchModel, optim_wrapper

    return TorchModel(model_fn=MlpNet, loss_fn=nn.CrossEntropyLoss, optim_fn=optim_wrapper(optim.Adam, lr=lr))


def _fl(aggregator, pyus, epochs=EPOCHS, hook=None, **kwargs):
    from sfl_amd.ml.fl import FLModel

    kwargs.setdefault("train_device", "cpu")
    fl = FLModel(server=None, device_list=pyus, model=_model(), aggregator=aggregator, strategy="fed_stc",
                 backend="torch", random_seed=1234, **kwargs)
    xs, ys = _data()
    hist = fl.fit({p: x for p, x in zip(pyus, xs)}, {p: y for p, y in zip(pyus, ys)}, batch_size=32, epochs=epochs,
                  aggregate_freq=1, validation_data=(np.concatenate(xs), np.concatenate(ys)), round_hook=hook)
    return fl, hist


def _is_ternary(t, max_nonzero):
    nz = t[t != 0]
    return nz.size <= max_nonzero and (nz.size == 0 or np.all(np.abs(nz) == np.abs(nz[0])))


def test_worker_step_by_hand():
    """One worker, one local step: the payload and the new residual split
    the dense update, and the model is back at its pre-step weights."""
    from sfl_amd.device import PYU
    from sfl_amd.ml.fl import FedAvgW, FedSTC

    xs, ys = _data()
    stc = FedSTC(_model(), PYU("client0", None), 1234, "cpu", sparsity=0.5)
    plain = FedAvgW(_model(), PYU("client0", None), 1234, "cpu")
    for w in (stc, plain):
        w.set_data(xs[0], ys[0], 32)
    before = stc.get_weights()
    assert all(np.array_equal(a, b) for a, b in zip(before, plain.get_weights()))
    payload, num = stc.train_step(None, 0, 1, refresh_data=True)
    after, num2 = plain.train_step(None, 0, 1, refresh_data=True)
    assert num == num2 == 32
    assert all(np.array_equal(a, b) for a, b in zip(before, stc.get_weights()))  # the local step is discarded
    for sparse, res, new, old in zip(payload, stc._res, after, before):
        u = np.subtract(new, old)
        m = round(0.5 * u.size)
        assert sparse.shape == u.shape and sparse.dtype == u.dtype == np.float32
        assert _is_ternary(sparse, u.size - m)
        # the residual is u - sparse exactly; adding it back gives u up to the two roundings of
        # (u - sparse) + sparse, each at most half a spacing at |u| + |sparse| (float addition
        # does not invert exactly: a small |u| under a large mu loses its last bits in u - mu)
        assert np.array_equal(res, np.subtract(u, sparse))
        assert np.all(np.abs(np.add(sparse, res) - u) <= np.spacing(np.abs(u) + np.abs(sparse)))
    # second step: the residual enters the update
    res1 = [r.copy() for r in stc._res]
    payload2, _ = stc.train_step(None, 1, 1)
    after2, _ = plain.train_step(before, 1, 1)  # from the same weights, the next batch
    for sparse, res, r1, new, old in zip(payload2, stc._res, res1, after2, before):
        u = np.add(np.subtract(new, old), r1)
        assert np.array_equal(res, np.subtract(u, sparse))


def test_fit_with_the_oracle_aggregator():
    from sfl_amd.device import PYU

    pyus = [PYU(n, None) for n in NAMES]
    agg = Recording(OracleAggregator(NAMES, o.seeds_for(NAMES)))
    down = []
    fl, hist = _fl(agg, pyus, hook=lambda r, p: down.append(p), sparsity=0.5)
    print("train_loss", hist["train_loss"], "val_accuracy", hist["val_accuracy"])
    assert len(agg.uploads) == 1 + 3 * EPOCHS
    for rnd in agg.uploads[1:]:  # [0] is the initial-weights average
        for party in rnd:
            for t in party:
                assert _is_ternary(t, t.size - round(0.5 * t.size))
    for upd in down[1:]:  # the server's downstream updates are ternary too
        for t in upd:
            assert t.dtype == np.float64 and _is_ternary(t, t.size - round(0.5 * t.size))
    w0 = fl.get_weights(pyus[0])
    for p in pyus[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(w0, fl.get_weights(p)))
    # the parties' float32 weights follow the server's float64 copy
    for w, s in zip(w0, fl.server_weight):
        assert np.allclose(w, s, rtol=0, atol=1e-5)
    assert hist["train_loss"][-1] < hist["train_loss"][0]


def test_no_sparsity_argument_means_rate_zero():
    from sfl_amd.device import PYU

    pyus = [PYU(n, None) for n in NAMES]
    agg = Recording(OracleAggregator(NAMES, o.seeds_for(NAMES)))
    fl, _ = _fl(agg, pyus, epochs=1)
    fl0, _ = _fl(OracleAggregator(NAMES, o.seeds_for(NAMES)), pyus, epochs=1, sparsity=0.0)
    for t in agg.uploads[1][0]:
        assert _is_ternary(t, t.size) and np.count_nonzero(t) > t.size // 2  # nothing masked: only exact zeros
    assert all(np.array_equal(a, b) for a, b in zip(fl.get_weights(), fl0.get_weights()))


def test_fed_stc_is_registered_and_checks_its_rate():
    from sfl_amd.device import PYU
    from sfl_amd.ml.fl import _STRATEGIES, FedSTC, FLModel

    assert _STRATEGIES[("fed_stc", "torch")] is FedSTC
    with pytest.raises(AssertionError):
        FLModel(device_list=[PYU("a", None)], model=_model(), aggregator=object(), strategy="fed_stc",
                train_device="cpu", sparsity=1.5)


@pytest.mark.gpu
def test_device_compression_oracle_vs_hip_aggregator_bit_exact():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sfl_amd.device import PYU
    from sfl_amd.security.aggregation import SecureAggregator

    seeds = o.seeds_for(NAMES)
    pair = {(a, b): seeds[a][b] for a in NAMES for b in NAMES if a != b}
    pyus = [PYU(n, 0) for n in NAMES]
    ref_down, hip_down = [], []
    ref = Recording(OracleAggregator(NAMES, seeds))
    hip = Recording(SecureAggregator(PYU("server", 0), pyus, seeds=pair))
    fl_ref, h_ref = _fl(ref, pyus, epochs=3, hook=lambda r, p: ref_down.append(p), sparsity=0.5,
                        compress_device="cuda:0")
    fl_hip, h_hip = _fl(hip, pyus, epochs=3, hook=lambda r, p: hip_down.append(p), sparsity=0.5,
                        compress_device="cuda:0")
    assert len(ref.aggregates) == len(hip.aggregates) == len(ref_down) == len(hip_down) == 1 + 3 * 3
    for r in range(len(ref_down)):
        for li, (x, y) in enumerate(zip(ref.aggregates[r], hip.aggregates[r])):
            assert x.dtype == y.dtype == np.float64 and np.array_equal(x, y), (r, li)
        for li, (x, y) in enumerate(zip(ref_down[r], hip_down[r])):
            assert np.array_equal(x, y), (r, li)
    for x, y in zip(fl_ref.get_weights(), fl_hip.get_weights()):
        assert np.array_equal(x, y)
    assert h_ref["val_accuracy"] == h_hip["val_accuracy"]


@pytest.mark.gpu
def test_device_compression_matches_numpy_on_the_first_round():
    """Later rounds may part by the last bit of mu (the two sums add in
    different orders) and are not compared."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sfl_amd.device import PYU

    pyus = [PYU(n, 0) for n in NAMES]
    host = Recording(OracleAggregator(NAMES, o.seeds_for(NAMES)))
    dev = Recording(OracleAggregator(NAMES, o.seeds_for(NAMES)))
    _fl(host, pyus, epochs=1, sparsity=0.5, compress_device="cpu")
    _fl(dev, pyus, epochs=1, sparsity=0.5, compress_device="cuda:0")
    for ph, pd in zip(host.uploads[1], dev.uploads[1]):
        for x, y in zip(ph, pd):
            assert x.dtype == y.dtype == np.float32
            assert np.array_equal(x != 0, y != 0) and np.array_equal(x < 0, y < 0)
            mx, my = np.abs(x).max(), np.abs(y).max()
            assert abs(float(mx) - float(my)) <= float(np.spacing(mx)), (mx, my)


@pytest.mark.gpu
def test_gpu_model_keeps_everything_on_the_device():
    """A GPU model compressed on its own GPU: the snapshot, the residual and
    the payload are device tensors, the aggregator takes them as they are,
    and the server's half runs on the aggregate's device in float64."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sfl_amd.device import PYU
    from sfl_amd.ml.fl import FedSTC
    from sfl_amd.security.aggregation import SecureAggregator

    xs, ys = _data()
    w = FedSTC(_model(), PYU("client0", 0), 1234, None, sparsity=0.9)
    w.set_data(xs[0], ys[0], 32)
    before = w.get_weights()
    for step in range(2):  # the second step has a residual
        payload, _ = w.train_step(None, step, 1, refresh_data=(step == 0))
        assert all(np.array_equal(a, b) for a, b in zip(before, w.get_weights()))
        for sparse, res, old in zip(payload, w._res, w.model_weights):
            assert sparse.is_cuda and res.is_cuda and old.is_cuda and sparse.dtype == torch.float32
            assert _is_ternary(_host(sparse), sparse.numel() - round(0.9 * sparse.numel()))
    seeds = o.seeds_for(NAMES)
    pair = {(a, b): seeds[a][b] for a in NAMES for b in NAMES if a != b}
    pyus = [PYU(n, 0) for n in NAMES]
    down = []
    fl, hist = _fl(SecureAggregator(PYU("server", 0), pyus, seeds=pair), pyus, epochs=2, sparsity=0.5,
                   train_device=None, hook=lambda r, p: down.append(p))
    for t in down[-1]:
        assert t.is_cuda and t.dtype == torch.float64
        assert _is_ternary(_host(t), t.numel() - round(0.5 * t.numel()))
    assert all(s.is_cuda and s.dtype == torch.float64 for s in fl.server_weight)
    w0 = fl.get_weights(pyus[0])
    for p in pyus[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(w0, fl.get_weights(p)))
    for a, s in zip(w0, fl.server_weight):
        assert np.allclose(a, _host(s), rtol=0, atol=1e-5)
