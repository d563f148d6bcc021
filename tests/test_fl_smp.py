"""``FLModel(strategy="fed_smp")`` on the CPU with the oracle aggregator: two
parties, two rounds.  Every upload is the by-hand FedSMP chain
(tests/smp_oracle.py) from the aggregate the parties received, the weights a
``fed_avg_w`` worker trains from it, and the mask whose key the documented
sequence gives."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

import smp_oracle as so  # noqa: E402
from oracle import secagg as o  # noqa: E402
from test_fl_round import MlpNet, OracleAggregator, _data  # noqa: E402
from test_fl_stc import Recording  # noqa: E402

NAMES = ["client0", "client1"]
SEED = 1234


def _model():
    from torch import optim

    from sfl_amd.ml.fl import TorchModel, optim_wrapper

    return TorchModel(model_fn=MlpNet, loss_fn=nn.CrossEntropyLoss, optim_fn=optim_wrapper(optim.Adam, lr=5e-3))


def _pyus():
    from sfl_amd.device import PYU

    return [PYU(n, None) for n in NAMES]


def _xy():
    xs, ys = _data(n_per=64)  # two batches of 32: two rounds per epoch
    return xs[:2], ys[:2]


def _fit(agg, pyus, hook=None, **kwargs):
    from sfl_amd.ml.fl import FLModel

    fl = FLModel(server=None, device_list=pyus, model=_model(), aggregator=agg, strategy="fed_smp", backend="torch",
                 random_seed=SEED, train_device="cpu", **kwargs)
    xs, ys = _xy()
    hist = fl.fit(dict(zip(pyus, xs)), dict(zip(pyus, ys)), batch_size=32, epochs=1, aggregate_freq=1, round_hook=hook)
    return fl, hist


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_fed_smp_is_accepted_and_sparse_transport_stays_refused():
    from sfl_amd.ml.fl import _STRATEGIES, FedSMP, FLModel

    assert _STRATEGIES[("fed_smp", "torch")] is FedSMP
    agg = OracleAggregator(NAMES, o.seeds_for(NAMES))
    fl = FLModel(server=None, device_list=_pyus(), model=_model(), aggregator=agg, strategy="fed_smp",
                 compression_ratio=0.25, train_device="cpu")
    assert all(w.compression_ratio == 0.25 for w in fl._workers.values())
    for st in ("down", "both"):
        with pytest.raises(ValueError, match="sparse_transport"):
            FLModel(server=None, device_list=_pyus(), model=_model(), aggregator=agg, strategy="fed_smp",
                    sparse_transport=st)
    with pytest.raises(AssertionError):
        FLModel(server=None, device_list=_pyus(), model=_model(), aggregator=agg, strategy="fed_smp",
                compression_ratio=1.5, train_device="cpu")


def test_a_worker_without_a_mask_refuses_and_takes_the_pair():
    from sfl_amd.ml.fl import FedSMP
    from sfl_amd.security.privacy import SMPMask

    xs, ys = _xy()
    w = FedSMP(_model(), _pyus()[0], SEED, "cpu", compression_ratio=0.5)
    w.set_data(xs[0], ys[0], 32)
    with pytest.raises(ValueError, match="no mask"):
        w.train_step(None, 0, 1, refresh_data=True)
    start = w.get_weights()
    mask = SMPMask(99, 0.5)
    up, n = w.train_step((start, mask), 0, 1, refresh_data=True)
    assert n == 32 and w.grad_mask == mask
    want = so.step(start, w.get_weights(), 99, 0.5)
    assert all(_same(a, b) for a, b in zip(up, want))
    w.apply_weights((start, SMPMask(100, 0.5)))
    assert w.grad_mask.key == 100 and all(_same(a, b) for a, b in zip(start, w.get_weights()))
    up2, _ = w.train_step(None, 1, 1)  # None: the weights and the mask the worker holds
    assert all(_same(a, b) for a, b in zip(up2, so.step(start, w.get_weights(), 100, 0.5)))


@pytest.mark.parametrize("p,clip", [(0.5, None), (0.5, 0.02), (1.0, None)], ids=["half", "half_clipped", "keep_all"])
def test_every_upload_is_the_by_hand_chain(p, clip):
    from sfl_amd.ml.fl import FedAvgW
    from sfl_amd.security.privacy import DPStrategyFL
    from sfl_amd.security.privacy.smp import mask_key

    pyus = _pyus()
    agg = Recording(OracleAggregator(NAMES, o.seeds_for(NAMES)))
    gdp = None if clip is None else so.clip_only(clip)
    down = []
    fl, hist = _fit(agg, pyus, hook=lambda r, a: down.append(a), compression_ratio=p,
                    dp_strategy=None if gdp is None else DPStrategyFL(model_gdp=gdp))
    assert len(agg.uploads) == len(down) == 3  # the initial average and two rounds
    assert hist["mask_bytes"] == [32, 32]  # 16 bytes per party and round
    # the server's masks: one with the initial average, one per aggregation, keys in the documented sequence
    assert [(m.key, m.ratio) for m in fl.masks] == [(mask_key(SEED, k), p) for k in range(3)]
    assert len({m.key for m in fl.masks}) == 3

    # a fed_avg_w worker per party replays the training: same seed, same data, same aggregate in
    xs, ys = _xy()
    shadows = [FedAvgW(_model(), d, SEED, "cpu") for d in pyus]
    for s, x, y in zip(shadows, xs, ys):
        s.set_data(x, y, 32)
    c = np.float32(p + 1e-6)
    for rnd in range(2):
        received = down[rnd]  # hook index -1 (the initial average) is down[0]
        key = mask_key(SEED, rnd)
        for i, s in enumerate(shadows):
            new, n = s.train_step(received, rnd, 1, refresh_data=(rnd == 0))  # fed_avg_w's upload
            old = [np.asarray(a).astype(np.float32) for a in received]  # what set_weights made of the aggregate
            want = so.step(old, new, key, p, gdp)
            got = agg.uploads[1 + rnd][i]
            assert all(_same(a, b) for a, b in zip(got, want)), (rnd, i)
            if p == 1.0:  # fed_avg_w's round bit for bit, but for the / c
                assert all(m.all() for m in so.masks(key, p, old))
                assert all(_same(a, o_ + (n_ - o_) / c) for a, o_, n_ in zip(got, old, new))
            else:
                kept = np.concatenate([m.reshape(-1) for m in so.masks(key, p, old)])
                same = np.concatenate([(a == b).reshape(-1) for a, b in zip(got, old)])
                assert same[~kept].all() and 0.3 < kept.mean() < 0.7
    # every party ends with the last aggregate
    w0 = fl.get_weights(pyus[0])
    assert all(np.array_equal(a, b) for a, b in zip(w0, fl.get_weights(pyus[1])))
    assert all(np.array_equal(a, np.asarray(b).astype(np.float32)) for a, b in zip(w0, down[-1]))


def test_without_a_seed_the_keys_come_from_the_os():
    from sfl_amd.ml.fl import FLModel

    pyus = _pyus()
    keys = []
    for _ in range(2):
        fl = FLModel(server=None, device_list=pyus, model=_model(), aggregator=OracleAggregator(NAMES, o.seeds_for(NAMES)),
                     strategy="fed_smp", train_device="cpu", compression_ratio=0.5)
        fl.initialize_weights()
        keys.append(fl.masks[0].key)
        assert all(w.grad_mask == fl.masks[0] for w in fl._workers.values())
    assert keys[0] != keys[1]


def test_the_other_strategies_send_what_they_sent():
    from sfl_amd.ml.fl import FLModel

    pyus = _pyus()
    fl = FLModel(server=None, device_list=pyus, model=_model(), aggregator=OracleAggregator(NAMES, o.seeds_for(NAMES)),
                 strategy="fed_avg_w", random_seed=SEED, train_device="cpu")
    xs, ys = _xy()
    hist = fl.fit(dict(zip(pyus, xs)), dict(zip(pyus, ys)), batch_size=32, epochs=1)
    assert "mask_bytes" not in hist and fl.masks == []
