"""The COO transport on the host: ``sparse_encode`` / ``sparse_decode``,
``SparsePlainAggregator`` and ``FLModel(sparse_transport=...)`` against the
numpy restatement (tests/coo_oracle.py), bit for bit.  The one convention:
where a numpy reduction can give ``-0.0`` and the zero-initialised
accumulator gives ``+0.0``, the reference is compared after ``ref + 0.0``."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

import coo_oracle as co  # noqa: E402
from oracle import secagg as o  # noqa: E402
from sfl_amd.device import PYU, PYUObject  # noqa: E402
from sfl_amd.security import SparsePlainAggregator  # noqa: E402
from sfl_amd.utils.compressor import SparseCOO, payload_nbytes, sparse_decode, sparse_encode  # noqa: E402
from test_fl_round import NAMES, MlpNet, OracleAggregator, _data  # noqa: E402
from test_fl_stc import Recording  # noqa: E402

SHAPES = {0: (), 1: (37,), 2: (5, 7), 4: (3, 2, 4, 3)}
DTYPES = (np.float32, np.float64, np.int64)


def _tensor(shape, dt, kind, seed=0):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape, dtype=np.int64))
    if kind == "zero":
        x = np.zeros(n)
    elif kind == "full":
        x = rng.integers(1, 9, n).astype(np.float64)
    else:
        x = rng.integers(-4, 5, n) * (rng.random(n) < 0.4)
    return x.astype(dt).reshape(shape)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("rank", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["mixed", "zero", "full"])
def test_host_round_trip(rank, dt, kind):
    x = _tensor(SHAPES[rank], dt, kind, seed=rank)
    (c,) = sparse_encode([x])
    idx, data = co.encode(x)
    assert isinstance(c, SparseCOO) and c.shape == x.shape and c.dtype == x.dtype
    assert c.index.dtype == np.int32 and np.array_equal(c.index, idx) and np.all(np.diff(c.index) > 0)
    assert c.data.dtype == x.dtype and np.array_equal(co.bits(c.data), co.bits(data))
    assert c.nnz == idx.size and c.nbytes == idx.size * (4 + x.dtype.itemsize)
    want = np.stack(np.nonzero(x)) if rank else co.coords(x)
    assert c.coords.dtype == np.int64 and c.coords.shape == (rank, idx.size) and np.array_equal(c.coords, want)
    (back,) = sparse_decode([c])
    assert back.dtype == x.dtype and back.shape == x.shape and np.array_equal(co.bits(back), co.bits(x + 0))
    assert np.array_equal(co.bits(c.todense()), co.bits(back))


def test_empty_tensors_and_cpu_tensors():
    for shape in ((0,), (0, 3), (2, 0, 4)):
        (c,) = sparse_encode([np.zeros(shape, np.float32)])
        assert c.nnz == 0 and c.nbytes == 0 and c.coords.shape == (len(shape), 0)
        assert sparse_decode([c])[0].shape == shape
    t = torch.tensor([[0.0, 2.0], [-1.0, 0.0]], dtype=torch.float64)
    n = torch.tensor(7)  # num_batches_tracked
    ct, cn = sparse_encode([t, n])
    assert ct.dtype == np.float64 and cn.dtype == np.int64 and cn.shape == () and cn.nnz == 1
    bt, bn = sparse_decode([ct, cn])
    assert isinstance(bt, torch.Tensor) and bt.dtype == torch.float64 and torch.equal(bt, t)
    assert isinstance(bn, torch.Tensor) and bn.dtype == torch.int64 and bn.shape == () and int(bn) == 7


@pytest.mark.parametrize("dt", (np.float32, np.float64), ids=["f32", "f64"])
def test_the_bit_rule(dt):
    tiny = np.nextafter(dt(0), dt(1))  # the smallest denormal
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny, 1.0, -0.0], dtype=dt)
    nan2 = np.array([0x7FC00123 if dt == np.float32 else 0x7FF8000000000123],
                    dtype=np.uint32 if dt == np.float32 else np.uint64).view(dt)
    x = np.concatenate([x, nan2])  # a NaN payload keeps its bits
    (c,) = sparse_encode([x])
    assert c.index.tolist() == [2, 3, 4, 5, 6, 7, 9]
    assert np.array_equal(co.bits(c.data), co.bits(x[c.index]))
    (back,) = sparse_decode([c])
    want = x.copy()
    want[[1, 8]] = 0.0  # -0.0 is dropped and decodes as +0.0
    assert np.array_equal(co.bits(back), co.bits(want))


def test_surface():
    assert sparse_encode(None) is None and sparse_decode(None) is None
    with pytest.raises(NotImplementedError):
        sparse_encode([np.ones(3)], encode_method="gcxs")
    with pytest.raises(AssertionError):
        sparse_encode([np.ones(3)], encode_method="csr")
    with pytest.raises(AssertionError):
        sparse_decode([np.ones(3)])
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4) * (np.arange(24).reshape(2, 3, 4) % 3 == 0)

    class Foreign:  # what sparse.COO offers
        coords, data, shape = np.stack(np.nonzero(x)), x[np.nonzero(x)], x.shape

    (back,) = sparse_decode([Foreign()])
    assert back.dtype == np.float32 and np.array_equal(back, x)
    assert payload_nbytes([x, sparse_encode([x])[0], torch.zeros(5, dtype=torch.float64)]) == \
        x.nbytes + 7 * 8 + 40
    assert payload_nbytes(None) == 0


def test_device_objects_move_sparse_entries():
    (c,) = sparse_encode([np.eye(3, dtype=np.float32)])
    moved = PYUObject(PYU("a", None), [c, np.ones(2)]).to(PYU("b", None)).data
    assert isinstance(moved[0], SparseCOO) and moved[0].index is not c.index and moved[0].data is not c.data
    assert np.array_equal(moved[0].index, c.index) and np.array_equal(moved[0].data, c.data)
    assert moved[0].shape == (3, 3) and moved[0].dtype == np.float32


# ---------------------------------------------------------------------------
# SparsePlainAggregator on host payloads
# ---------------------------------------------------------------------------
LAYERS = ((16, 9), (9,), (2, 3, 2, 2), (1,))  # the one-element layer: numpy sums it pairwise from 8 parties on


def _parties(K, dt, support, seed=0):
    """K per-layer lists: overlapping, disjoint or empty supports."""
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
            else:
                keep = np.zeros(n, dtype=bool)
            layers.append(np.where(keep, v, dt(0)).reshape(shape))
        out.append(layers)
    return out


def _weights(kind, K):
    if kind == "int":
        return [32 + 7 * k for k in range(K)]
    if kind == "f64":
        return list(np.random.default_rng(K).random(K) + 1.0)
    return None


def _objs(parties, sparse):
    pyus = [PYU(f"p{k}", None) for k in range(len(parties))]
    return [PYUObject(p, sparse_encode(layers) if sparse else layers) for p, layers in zip(pyus, parties)]


@pytest.mark.parametrize("dt", (np.float32, np.float64), ids=["f32", "f64"])
@pytest.mark.parametrize("support", ["overlap", "disjoint", "empty"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_aggregator_equals_numpy(K, support, dt):
    agg = SparsePlainAggregator(PYU("server", None))
    parties = _parties(K, dt, support)
    for axis in (0, None, 1):
        if axis == 1 and K != 2:
            continue  # one representative: other axes go through numpy itself
        got = agg.sum(_objs(parties, True), axis=axis).data
        for li in range(len(LAYERS)):
            if axis == 1 and parties[0][li].ndim < 1:
                continue
            ref = co.total([p[li] for p in parties], axis=axis)
            assert co.same_bits(got[li], ref), ("sum", axis, li)
        for wk in ("int", "f64", None):
            w = _weights(wk, K)
            if axis != 0 and w is not None:
                continue  # numpy wants weights of the full shape there
            got = agg.average(_objs(parties, True), axis=axis, weights=w).data
            for li in range(len(LAYERS)):
                ref = co.average([p[li] for p in parties], axis=axis, weights=w)
                assert co.same_bits(got[li], ref), ("average", axis, wk, li)


def test_aggregator_single_entries_and_mixed_lists():
    agg = SparsePlainAggregator(PYU("server", None))
    parties = _parties(3, np.float32, "overlap")
    w = [3, 1, 2]
    dense = agg.average(_objs(parties, False), axis=0, weights=w).data
    mixed_objs = _objs(parties, True)
    mixed_objs[1] = _objs(parties, False)[1]
    mixed = agg.average(mixed_objs, axis=0, weights=w).data
    sparse = agg.average(_objs(parties, True), axis=0, weights=w).data
    for d, m, s, li in zip(dense, mixed, sparse, range(len(LAYERS))):
        assert co.same_bits(m, d) and co.same_bits(s, d)
        assert co.same_bits(d, co.average([p[li] for p in parties], axis=0, weights=w))
    # a single entry per party instead of a per-layer list
    singles = [PYUObject(PYU(f"p{k}", None), sparse_encode([p[0]])[0]) for k, p in enumerate(parties)]
    assert co.same_bits(agg.sum(singles, axis=0).data, co.total([p[0] for p in parties], axis=0))
    assert agg.accepts_sparse and "debugging" in SparsePlainAggregator.__doc__


def _malformed():
    good = sparse_encode([np.arange(1.0, 11.0, dtype=np.float32)])[0]
    bad = {}
    for name, index in (("range", [0, 3, 10]), ("order", [0, 5, 3]), ("duplicate", [2, 4, 4])):
        bad[name] = SparseCOO(good.shape, good.dtype, np.array(index, np.int32), np.ones(3, np.float32))
    return good, bad


@pytest.mark.parametrize("what", ["range", "order", "duplicate"])
def test_malformed_payloads_are_refused(what):
    good, bad = _malformed()
    with pytest.raises(ValueError, match=r"\[1\]"):
        sparse_decode([good, bad[what]])
    agg = SparsePlainAggregator(PYU("server", None))
    data = [PYUObject(PYU("a", None), [good]), PYUObject(PYU("b", None), [bad[what]])]
    for axis in (0, None):
        with pytest.raises(ValueError, match="layer 0"):
            agg.sum(data, axis=axis)
        with pytest.raises(ValueError, match="layer 0"):
            agg.average(data, axis=axis)
    with pytest.raises(ValueError):
        sparse_decode([SparseCOO((10,), np.float32, np.array([-1], np.int32), np.ones(1, np.float32))])


# ---------------------------------------------------------------------------
# FLModel
# ---------------------------------------------------------------------------
PARTIES = NAMES[:2]


def _fl(aggregator, strategy="fed_stc", epochs=2, **kwargs):
    from torch import optim

    from sfl_amd.ml.fl import FLModel, TorchModel, optim_wrapper

    lr, opt = (5e-3, optim.Adam) if strategy != "fed_scr" else (0.3, optim.SGD)
    model = TorchModel(model_fn=MlpNet, loss_fn=nn.CrossEntropyLoss, optim_fn=optim_wrapper(opt, lr=lr))
    pyus = [PYU(n, None) for n in PARTIES]
    fl = FLModel(server=None, device_list=pyus, model=model, aggregator=aggregator, strategy=strategy,
                 backend="torch", random_seed=1234, train_device="cpu", **kwargs)
    xs, ys = _data()
    down = []
    hist = fl.fit({p: x for p, x in zip(pyus, xs)}, {p: y for p, y in zip(pyus, ys)}, batch_size=32, epochs=epochs,
                  aggregate_freq=1, round_hook=lambda r, p: down.append([np.array(t, copy=True) for t in p]))
    return fl, hist, down


class SparseRecording(Recording):
    """``Recording`` for uploads that may be sparse: it keeps them decoded."""

    accepts_sparse = True

    def average(self, data, axis=0, weights=None):
        self.uploads.append([[np.array(x.todense() if isinstance(x, SparseCOO) else x, copy=True) for x in d.data]
                             for d in data])
        self.raw = [d.data for d in data]
        out = self.inner.average(data, axis=axis, weights=weights)
        self.aggregates.append([np.array(x, copy=True) for x in out.data])
        return out


def _same_run(a, b):
    (fl_a, _, down_a), (fl_b, _, down_b) = a, b
    assert len(down_a) == len(down_b) == 1 + 2 * 3
    for r, (x, y) in enumerate(zip(down_a, down_b)):
        for li, (s, t) in enumerate(zip(x, y)):
            assert s.dtype == t.dtype and np.array_equal(co.bits(s + 0.0), co.bits(t + 0.0)), (r, li)
    for p in PARTIES:
        for s, t in zip(fl_a.get_weights(PYU(p, None)), fl_b.get_weights(PYU(p, None))):
            assert np.array_equal(co.bits(s), co.bits(t))


def test_fl_both_equals_the_dense_run():
    dense_agg = SparseRecording(SparsePlainAggregator(PYU("server", None)))
    both_agg = SparseRecording(SparsePlainAggregator(PYU("server", None)))
    dense = _fl(dense_agg, sparsity=0.9)
    both = _fl(both_agg, sparsity=0.9, sparse_transport="both")
    assert all(isinstance(x, SparseCOO) for party in both_agg.raw for x in party)
    for r, (x, y) in enumerate(zip(dense_agg.aggregates, both_agg.aggregates)):
        for li, (s, t) in enumerate(zip(x, y)):
            assert s.dtype == t.dtype and np.array_equal(co.bits(s + 0.0), co.bits(t + 0.0)), (r, li)
    _same_run(dense, both)
    hist_d, hist_b = dense[1], both[1]
    assert "upload_bytes" not in hist_d and "download_bytes" not in hist_d
    assert set(hist_b) == set(hist_d) | {"upload_bytes", "download_bytes"}
    assert len(hist_b["upload_bytes"]) == len(hist_b["download_bytes"]) == 2 * 3
    for r, up in enumerate(hist_b["upload_bytes"]):
        dense_bytes = sum(payload_nbytes(party) for party in dense_agg.uploads[1 + r])
        n = sum(t.size for t in dense_agg.uploads[1 + r][0])
        print(f"round {r}: sparse upload {up} B, dense {dense_bytes} B")
        assert up < dense_bytes and dense_bytes == len(PARTIES) * n * 4
        # at most n - round(0.9 n) entries of 8 bytes per layer
        assert up <= len(PARTIES) * sum((t.size - round(0.9 * t.size)) * 8 for t in dense_agg.uploads[1 + r][0])
    for r, dn in enumerate(hist_b["download_bytes"]):
        assert dn <= len(PARTIES) * sum((t.size - round(0.9 * t.size)) * 12 for t in dense_agg.uploads[1][0])


def test_fl_down_with_the_oracle_aggregator():
    dense = _fl(OracleAggregator(PARTIES, o.seeds_for(PARTIES)), sparsity=0.9)
    down = _fl(OracleAggregator(PARTIES, o.seeds_for(PARTIES)), sparsity=0.9, sparse_transport="down")
    _same_run(dense, down)
    n = sum(w.size for w in dense[0].get_weights())
    assert all(b == len(PARTIES) * n * 4 for b in down[1]["upload_bytes"])  # dense uploads
    assert all(b < len(PARTIES) * n * 8 * 0.2 for b in down[1]["download_bytes"])


def test_fl_scr_both_equals_the_dense_run():
    dense_agg = SparseRecording(SparsePlainAggregator(PYU("server", None)))
    both_agg = SparseRecording(SparsePlainAggregator(PYU("server", None)))
    dense = _fl(dense_agg, strategy="fed_scr", threshold=0.5)
    both = _fl(both_agg, strategy="fed_scr", threshold=0.5, sparse_transport="both")
    assert all(isinstance(x, SparseCOO) for party in both_agg.raw for x in party)
    assert any(np.count_nonzero(t) < t.size for t in dense_agg.uploads[1][0])  # something was pruned
    _same_run(dense, both)
    assert all(isinstance(t, np.ndarray) for t in both[2][-1])  # fed_scr's downstream stays dense


def test_fl_refuses_what_cannot_work():
    from sfl_amd.ml.fl import FLModel, TorchModel

    model = TorchModel(model_fn=MlpNet, loss_fn=nn.CrossEntropyLoss, optim_fn=lambda p: torch.optim.SGD(p, lr=0.1))
    pyus = [PYU(n, None) for n in PARTIES]
    common = dict(server=None, device_list=pyus, model=model, train_device="cpu", random_seed=1)
    with pytest.raises(ValueError, match="masks every element"):
        FLModel(aggregator=OracleAggregator(PARTIES, o.seeds_for(PARTIES)), strategy="fed_stc", sparsity=0.9,
                sparse_transport="both", **common)
    with pytest.raises(ValueError, match="fed_avg_w"):
        FLModel(aggregator=SparsePlainAggregator(PYU("server", None)), strategy="fed_avg_w",
                sparse_transport="both", **common)
    with pytest.raises(ValueError):
        FLModel(aggregator=SparsePlainAggregator(PYU("server", None)), strategy="fed_stc", sparsity=0.9,
                sparse_transport="up", **common)
