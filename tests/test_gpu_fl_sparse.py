"""``FLModel(sparse_transport=...)`` with models resident on the GPU: the
uploads of ``fed_stc`` / ``fed_scr`` are device ``SparseCOO``s, the server
sums them on the device, and every setting gives the dense run's weights bit
for bit (the sign of a zero apart)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

import coo_oracle as co  # noqa: E402
from gpu_copies import _host  # noqa: E402
from oracle import secagg as o  # noqa: E402
from sfl_amd.device import PYU  # noqa: E402
from sfl_amd.security import SparsePlainAggregator  # noqa: E402
from sfl_amd.utils.sparse import SparseCOO  # noqa: E402
from test_fl_round import NAMES, MlpNet, OracleAggregator, _data  # noqa: E402

pytestmark = pytest.mark.gpu
PARTIES = NAMES[:2]
ROUNDS = 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(x):
    """A host copy of an upload or an aggregate, wherever it lives (pinned copies only)."""
    if isinstance(x, SparseCOO):
        return np.array(x.to("cpu").todense(), copy=True)
    if isinstance(x, torch.Tensor):
        return _host(x) if x.is_cuda else x.numpy().copy()
    return np.array(x, copy=True)


class Recording:
    """An aggregator that keeps what went into ``average``, as it came and on the host."""

    accepts_sparse = True

    def __init__(self, inner):
        self.inner, self.raw, self.uploads = inner, [], []

    def average(self, data, axis=0, weights=None):
        self.raw.append([list(d.data) for d in data])
        self.uploads.append([[_np(x) for x in d.data] for d in data])
        return self.inner.average(data, axis=axis, weights=weights)


def _run(strategy, transport, **kwargs):
    """Two rounds on GPU models: (FLModel, history, aggregator, per-round aggregates, per-round server weights,
    every party's weights after each round)."""
    from torch import optim

    from sfl_amd.ml.fl import FLModel, TorchModel, optim_wrapper

    lr, opt = (5e-3, optim.Adam) if strategy != "fed_scr" else (0.3, optim.SGD)
    model = TorchModel(model_fn=MlpNet, loss_fn=nn.CrossEntropyLoss, optim_fn=optim_wrapper(opt, lr=lr))
    pyus = [PYU(n, 0) for n in PARTIES]
    agg = Recording(SparsePlainAggregator(PYU("server", 0)))
    fl = FLModel(server=None, device_list=pyus, model=model, aggregator=agg, strategy=strategy, backend="torch",
                 random_seed=1234, train_device="cuda:0", sparse_transport=transport, **kwargs)
    assert all(w._resident for w in fl._workers.values())
    xs, ys = _data(n_per=32 * ROUNDS)
    down, server, held = [], [], []

    def hook(r, p):
        down.append([_np(t) for t in p])
        if strategy == "fed_stc" and r >= 0:
            server.append([_np(t) for t in fl.server_weight])
        if r >= 0:  # what the party holds when the round ends (the round's update reaches it with the next step)
            held.append([w.get_weights() for w in fl._workers.values()])

    hist = fl.fit({p: x for p, x in zip(pyus, xs)}, {p: y for p, y in zip(pyus, ys)}, batch_size=32, epochs=1,
                  aggregate_freq=1, round_hook=hook)
    return fl, hist, agg, down, server, held


_runs = {}


def _cached(strategy, transport):
    if (strategy, transport) not in _runs:
        kw = {"sparsity": 0.9} if strategy == "fed_stc" else {"threshold": 0.5}
        _runs[(strategy, transport)] = _run(strategy, transport, **kw)
    return _runs[(strategy, transport)]


def _same_lists(a, b, what):
    assert len(a) == len(b), what
    for li, (s, t) in enumerate(zip(a, b)):
        assert s.dtype == t.dtype and s.shape == t.shape, (what, li)
        assert np.array_equal(co.bits(s + 0.0), co.bits(t + 0.0)), (what, li)  # +-0 apart


def _same_run(a, b, what):
    (fl_a, _, _, down_a, srv_a, held_a), (fl_b, _, _, down_b, srv_b, held_b) = a, b
    assert len(down_a) == len(down_b) == 1 + ROUNDS
    for r, (x, y) in enumerate(zip(down_a, down_b)):
        _same_lists(x, y, (what, "aggregate", r))
    assert len(srv_a) == len(srv_b)
    for r, (x, y) in enumerate(zip(srv_a, srv_b)):
        _same_lists(x, y, (what, "server weights", r))
    assert len(held_a) == len(held_b) == ROUNDS
    for r, (x, y) in enumerate(zip(held_a, held_b)):
        for k, (s, t) in enumerate(zip(x, y)):
            _same_lists(s, t, (what, "party weights after round", r, k))
    for p in PARTIES:
        _same_lists(fl_a.get_weights(PYU(p, 0)), fl_b.get_weights(PYU(p, 0)), (what, "weights", p))


@pytest.mark.parametrize("transport", ["down", "both"])
def test_fed_stc_equals_the_dense_run(transport):
    dense, sparse = _cached("fed_stc", None), _cached("fed_stc", transport)
    assert len(dense[4]) == ROUNDS
    _same_run(dense, sparse, transport)
    hist = sparse[1]
    assert "upload_bytes" not in dense[1]
    assert len(hist["upload_bytes"]) == len(hist["download_bytes"]) == ROUNDS
    if transport == "down":
        n = sum(t.size for t in dense[2].uploads[1][0])
        assert all(b == len(PARTIES) * n * 4 for b in hist["upload_bytes"])  # dense uploads
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for party in sparse[2].raw[1] for x in party)


def test_both_uploads_device_coos_and_counts_their_bytes():
    dense, both = _cached("fed_stc", None), _cached("fed_stc", "both")
    for rnd in both[2].raw[1:]:  # raw[0] is the average of the initial weights
        assert all(isinstance(x, SparseCOO) and x.is_device and x.index.is_cuda and x.data.is_cuda
                   for party in rnd for x in party)
    for r, up in enumerate(both[1]["upload_bytes"]):
        want = sum(int(np.count_nonzero(co.nonzero_mask(t.reshape(-1)))) * (4 + t.dtype.itemsize)
                   for party in dense[2].uploads[1 + r] for t in party)
        dense_bytes = sum(t.nbytes for party in dense[2].uploads[1 + r] for t in party)
        print(f"round {r}: sparse upload {up} B, dense {dense_bytes} B")
        assert up == want and 0 < up < dense_bytes
    # the downstream update is sparse too: at most n - round(0.9 n) entries of 12 bytes (float64) per layer
    cap = len(PARTIES) * sum((t.size - round(0.9 * t.size)) * 12 for t in dense[2].uploads[1][0])
    assert all(0 < dn <= cap for dn in both[1]["download_bytes"])


def test_fed_scr_both_equals_the_dense_run():
    dense, both = _cached("fed_scr", None), _cached("fed_scr", "both")
    _same_run(dense, both, "fed_scr both")
    for rnd in both[2].raw[1:]:
        assert all(isinstance(x, SparseCOO) and x.is_device for party in rnd for x in party)
    assert any(np.count_nonzero(t) < t.size for t in dense[2].uploads[1][0])  # something was pruned
    for r, up in enumerate(both[1]["upload_bytes"]):
        want = sum(int(np.count_nonzero(co.nonzero_mask(t.reshape(-1)))) * (4 + t.dtype.itemsize)
                   for party in dense[2].uploads[1 + r] for t in party)
        assert up == want


def test_fl_refuses_what_cannot_work_on_a_gpu_model():
    from sfl_amd.ml.fl import FLModel, TorchModel

    model = TorchModel(model_fn=MlpNet, loss_fn=nn.CrossEntropyLoss, optim_fn=lambda p: torch.optim.SGD(p, lr=0.1))
    pyus = [PYU(n, 0) for n in PARTIES]
    common = dict(server=None, device_list=pyus, model=model, train_device="cuda:0", random_seed=1)
    # what raised ValueError for a resident worker now succeeds
    fl = FLModel(aggregator=SparsePlainAggregator(PYU("server", 0)), strategy="fed_stc", sparsity=0.9,
                 sparse_transport="both", **common)
    assert all(w._resident for w in fl._workers.values())
    with pytest.raises(ValueError, match="masks every element"):
        FLModel(aggregator=OracleAggregator(PARTIES, o.seeds_for(PARTIES)), strategy="fed_stc", sparsity=0.9,
                sparse_transport="both", **common)
    with pytest.raises(ValueError, match="fed_avg_w"):
        FLModel(aggregator=SparsePlainAggregator(PYU("server", 0)), strategy="fed_avg_w",
                sparse_transport="both", **common)
    with pytest.raises(ValueError):
        FLModel(aggregator=SparsePlainAggregator(PYU("server", 0)), strategy="fed_stc", sparsity=0.9,
                sparse_transport="up", **common)
