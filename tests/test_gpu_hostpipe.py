"""sfl_amd/hostpipe.py's one-shot host copies on the GPU: ``d2h`` / ``h2d``
(no pageable DMA: pooled registered buffers or pinned staging) round-trip
every element type, shape and placement the product hands them, bit for
bit; and ``run_chunks``, the driver of the chunked calls, on a stand-in
compute step: its result, and the order in which it drains the streams,
joins its threads and unregisters the inputs when a step fails."""
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from gpu_copies import _dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


CASES = [
    (np.float32, (3_000_001,)),  # 12 MB: a pooled result
    (np.float64, (1001, 997)),
    (np.int64, (2_000_003,)),
    (np.int32, (17,)),
    (np.float16, (4, 5, 6)),
    (np.bool_, (1000,)),
    (np.float64, ()),
    (np.float32, (0,)),
]


@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("dt,shape", CASES)
def test_d2h_h2d_round_trip(dt, shape, pooled, monkeypatch):
    from sfl_amd import hostpipe as H

    monkeypatch.setattr(H, "RESULTS", H.ResultPool(1 << 30))
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(shape) * 1e3).astype(dt) if dt != np.bool_ else rng.random(shape) < 0.5
    dev = torch.device("cuda", 0)
    t = H.h2d(a, dev)
    assert t.device == dev and tuple(t.shape) == shape
    back = H.d2h(t, pooled=pooled)
    assert back.dtype == np.dtype(dt) and back.shape == shape
    assert np.array_equal(back.reshape(-1).view(np.uint8), np.ascontiguousarray(a).reshape(-1).view(np.uint8))
    if pooled and a.nbytes >= 8 << 20:
        assert H.RESULTS.contains(back)  # straight into a registered buffer
    else:
        assert not H.RESULTS.contains(back)
    del back
    H.RESULTS.clear()


def test_d2h_h2d_views_tensors_and_u64(monkeypatch):
    from sfl_amd import hostpipe as H

    monkeypatch.setattr(H, "RESULTS", H.ResultPool(1 << 30))
    dev = torch.device("cuda", 0)
    base = torch.arange(4_000_000, dtype=torch.int64, device=dev).reshape(2000, 2000)
    view = base.t()[::2]  # non-contiguous device view
    assert np.array_equal(H.d2h(view), np.arange(4_000_000, dtype=np.int64).reshape(2000, 2000).T[::2])
    # uint64 host arrays (masked vectors) go up as their int64 bits
    u = np.arange(2**64 - 1000, 2**64 - 1, dtype=np.uint64)
    t = H.h2d(u, dev)
    assert t.dtype == torch.int64 and np.array_equal(H.d2h(t).view(np.uint64), u)
    # a CPU tensor is a host array; a device tensor is moved as it is
    x = torch.randn(300_001)
    assert np.array_equal(H.d2h(H.h2d(x, dev), pooled=False), x.numpy())
    y = torch.randn(10, device=dev)
    assert H.h2d(y, dev).data_ptr() == y.data_ptr()
    # an array inside a pooled result is copied as it is (already registered)
    owner = H.RESULTS.take(16 << 20)
    pooled = owner[: 8 << 20].view(np.float64)
    pooled[:] = np.arange(pooled.size)
    assert np.array_equal(H.d2h(H.h2d(pooled[5:], dev), pooled=False), pooled[5:])
    with pytest.raises(TypeError, match="no host array type"):
        H.d2h(torch.zeros(3, dtype=torch.bfloat16, device=dev))
    del owner, pooled
    H.RESULTS.clear()


def test_gpu_model_weights_round_trip_without_pageable_copies():
    """FedAvgW on a GPU model: get_weights (hostpipe.d2h) and set_weights
    from numpy arrays, CPU tensors and device tensors (hostpipe.h2d or a
    device copy) give back the same bits; a float64 array loads into the
    float32 parameters as the reference's torch.Tensor(np.copy(v)) does."""
    from torch import nn, optim

    from sfl_amd.device import PYU
    from sfl_amd.ml.fl import FedAvgW, TorchModel, optim_wrapper

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = nn.Linear(1000, 3000)  # 12 MB of weights: a pooled-size array
            self.b = nn.Linear(3000, 7)

    torch.manual_seed(0)
    m = TorchModel(model_fn=Net, loss_fn=nn.CrossEntropyLoss, optim_fn=optim_wrapper(optim.SGD, lr=0.1))
    w = FedAvgW(m, PYU("alice", 0))
    assert next(w.model.parameters()).is_cuda
    ws = w.get_weights()
    assert [a.dtype for a in ws] == [np.float32] * 4
    # the weights were initialised on the device: compared there, each array sent back up
    assert all(torch.equal(_dev(a).reshape(a.shape), p) for a, p in zip(ws, w.model.state_dict().values()))
    for form in ("numpy", "cpu", "cuda", "f64"):
        new = [np.asarray(a) * 2 + 1 for a in ws]
        give = {"numpy": new, "cpu": [torch.from_numpy(a) for a in new],
                "cuda": [_dev(a).reshape(a.shape) for a in new],
                "f64": [a.astype(np.float64) for a in new]}[form]
        w.set_weights(give)
        got = w.get_weights()
        assert all(np.array_equal(g, a.astype(np.float32)) for g, a in zip(got, new)), form
        td = w.get_weights(return_numpy=False)
        assert all(t.device.type == "cpu" and np.array_equal(t.numpy(), g) for t, g in zip(td.values(), got)), form


# ---------------------------------------------------------------- run_chunks
# the smallest call with three uneven chunks and a layer join (1500) inside
# one of them; 20 kB of result: never a pooled buffer, so every chunk goes
# through a pinned slot and the drain thread
N, BOUNDS = 2500, [(0, 1024), (1024, 2048), (2048, 2500)]


@pytest.fixture(scope="module")
def layers():
    """Two float32 host layers of 1500 and 1000 elements, each on pages of
    its own (so each can be registered whatever else the heap holds), and
    twice their concatenation as float64."""
    raw = np.empty(4 * 4096, dtype=np.uint8)
    off = -raw.ctypes.data % 4096
    a, b = raw[off:off + 6000].view(np.float32), raw[off + 8192:off + 12192].view(np.float32)
    rng = np.random.default_rng(11)
    a[:], b[:] = rng.standard_normal(1500), rng.standard_normal(1000)
    return [a, b], 2 * np.concatenate([a, b]).astype(np.float64)


def _double(H, layers, seen, fail_at=None, error=None):
    """``run_chunks`` with ``dec = 2 * x`` as the compute step and a device
    counter of the steps as the meta word; ``seen`` collects the chunks the
    step was called for, and chunk ``fail_at``'s call raises ``error``."""
    dev = torch.device("cuda", 0)

    def setup():
        x = torch.empty(N, dtype=torch.float32, device=dev)
        dec = torch.empty(N, dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)

        def compute(j, lo, hi):
            seen.append(j)
            if j == fail_at:
                raise error
            dec[lo:hi] = x[lo:hi].double() * 2
            count.add_(1)

        copies = [[(x[lo:hi], H.pieces(layers, lo, hi))] for lo, hi in BOUNDS]
        return copies, compute, lambda j: dec[BOUNDS[j][0]:BOUNDS[j][1]], count

    return H.run_chunks("double", dev, BOUNDS, layers, np.float64, setup)


def _feeds(H, monkeypatch):
    """The names of the feeders ``run_chunks`` builds from here on."""
    made = []
    for name in ("Issued", "Feeder"):
        monkeypatch.setattr(H, name, lambda *a, _cls=getattr(H, name), _name=name: made.append(_name) or _cls(*a))
    return made


def _no_helper_threads():
    return not [t.name for t in threading.enumerate() if t.name in ("sfl_sa_h2d", "sfl_sa_d2h")]


def _normal_call_is_exact(H, layers, want):
    seen = []
    got, meta = _double(H, layers, seen)
    return np.array_equal(got, want) and meta.tolist() == [3] and seen == [0, 1, 2]


@pytest.mark.parametrize("pinned", [True, False])
def test_run_chunks_round_trip(pinned, layers, monkeypatch):
    from test_gpu_party_pipeline import _NotPinned

    from sfl_amd import hostpipe as H

    layers, want = layers
    if not pinned:
        monkeypatch.setattr(H, "Pinned", _NotPinned)
    made, seen = _feeds(H, monkeypatch), []
    got, meta = _double(H, layers, seen)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert meta.dtype == np.int64 and meta.tolist() == [3]
    assert seen == [0, 1, 2]
    assert made == (["Issued"] if pinned else ["Feeder"])  # registered inputs: async DMA; else the feeder thread
    assert _no_helper_threads()


def test_run_chunks_compute_error_drains_before_unregistering(layers, monkeypatch):
    """The compute step raises at chunk 1 (chunk 0's D2H and chunk 2's H2D
    are in flight): the caller gets that exception, after the three streams
    were synchronised and only then the inputs unregistered, once."""
    from sfl_amd import hostpipe as H

    layers, want = layers
    order = []
    names = dict(zip(H.streams(torch.device("cuda", 0)), ("h2d", "compute", "d2h")))
    sync, exit_ = torch.cuda.Stream.synchronize, H.Pinned.__exit__

    def spy_sync(self):
        sync(self)
        if self in names:
            order.append("sync " + names[self])

    def spy_exit(self, *exc):
        order.append("unregister")
        return exit_(self, *exc)

    boom, seen = RuntimeError("compute step failed"), []
    with monkeypatch.context() as m:
        m.setattr(torch.cuda.Stream, "synchronize", spy_sync)
        m.setattr(H.Pinned, "__exit__", spy_exit)
        with pytest.raises(RuntimeError) as ei:
            _double(H, layers, seen, fail_at=1, error=boom)
    assert ei.value is boom
    assert seen == [0, 1]
    assert order == ["sync compute", "sync d2h", "sync h2d", "unregister"]
    assert _no_helper_threads()
    assert _normal_call_is_exact(H, layers, want)


def test_run_chunks_feeder_error_reaches_the_caller(layers, monkeypatch):
    """The feeder thread fails staging the second layer (chunk 1 holds the
    join): its exception is raised in the caller from the chunk loop, both
    helper threads are joined, and the next call is exact."""
    from test_gpu_party_pipeline import _NotPinned

    from sfl_amd import hostpipe as H

    layers, want = layers
    pcopy, boom, seen = H.pcopy, RuntimeError("staging failed"), []

    def failing(dst, src):  # the drain thread's copies (out of a pinned slot) pass
        if np.shares_memory(src, layers[1]):
            raise boom
        pcopy(dst, src)

    with monkeypatch.context() as m:
        m.setattr(H, "Pinned", _NotPinned)
        m.setattr(H, "pcopy", failing)
        made = _feeds(H, m)
        with pytest.raises(RuntimeError) as ei:
            _double(H, layers, seen)
    assert ei.value is boom and made == ["Feeder"]
    # chunk 0 ran unless the feeder had failed before the loop asked for it; the chunk it failed on never did
    assert seen in ([], [0])
    assert _no_helper_threads()
    assert _normal_call_is_exact(H, layers, want)
