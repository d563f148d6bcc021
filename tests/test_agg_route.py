"""Which route a SecureAggregator call takes (``SecureAggregator._route``, the
table in DESIGN.md §7): one case per row and both sides of every boundary.
The decision is pure Python on the call's fields, so nothing here touches a
GPU."""
import numpy as np
import pytest

from sfl_amd.device import PYU, PYUObject
from sfl_amd.security.aggregation import SecureAggregator
from sfl_amd.security.aggregation import party as P
from sfl_amd.security.aggregation.payload import F32, F64, compute_dtype


def _route(payload, C=3, weights=None, careful=False, gpus=None, **kw):
    """(route, call) of C parties that each hold ``payload``."""
    names = [f"p{i:02d}" for i in range(C)]
    pyus = [PYU(nm, 0 if gpus is None else gpus[i]) for i, nm in enumerate(names)]
    seeds = {(a, b): 1000 * i + j for i, a in enumerate(names) for j, b in enumerate(names) if a < b}
    agg = SecureAggregator(PYU("server", 0), pyus, seeds=seeds, **kw)
    agg._careful = careful
    call = agg._build_call([PYUObject(p, payload) for p in pyus], weights, weights is not None)
    return agg._route(call), call


def _arr(n, dtype=np.float32):
    return np.zeros(n, dtype=dtype)


@pytest.mark.parametrize("n,pipeline,want", [(262_144, True, "fused_one_call"), (262_145, True, "fused_pipelined"),
                                             (262_145, False, "fused_staged"), (262_144, False, "fused_one_call")])
def test_float32_size_boundary(n, pipeline, want, monkeypatch):
    """4 * n_pad against SMALL_CALL_BYTES (n_pad: n rounded up to 4)."""
    monkeypatch.setattr(P, "LARGE_PIPELINE", pipeline)
    assert _route(_arr(n))[0] == want


@pytest.mark.parametrize("C,careful,want", [(2, False, "fused_one_call"), (8, False, "fused_one_call"),
                                            (9, False, "fused_staged"), (8, True, "fused_staged"),
                                            (9, True, "general")])
def test_float32_party_cap_and_careful_replay(C, careful, want):
    """sa_fused_clients_host_f32 takes 2..8 parties; a replay is staged from
    Python, and with more than 8 parties it leaves the fused routes."""
    assert _route(_arr(99), C=C, careful=careful)[0] == want


def test_float32_large_careful_replay_is_staged():
    assert _route(_arr(262_145), careful=True)[0] == "fused_staged"


@pytest.mark.parametrize("dtype", [np.float64, np.int64])
@pytest.mark.parametrize("n,pipeline,want", [(131_072, True, "general_one_call"), (131_073, True, "general_pipelined"),
                                             (131_073, False, "general")])
def test_general_size_boundary(dtype, n, pipeline, want, monkeypatch):
    """n * itemsize against SMALL_CALL_BYTES."""
    monkeypatch.setattr(P, "LARGE_PIPELINE", pipeline)
    assert _route(_arr(n, dtype))[0] == want


def test_general_party_cap():
    """sa_clients_host takes 2..9 parties; beyond it a layer list is packed
    on the host and a single array goes to the general path."""
    two = [np.zeros((3, 5), dtype=np.int64), np.zeros(7, dtype=np.int64)]
    assert _route(two, C=9)[0] == "general_one_call"
    assert _route(two, C=10)[0] == "general_host_packed"
    assert _route(two[0], C=10)[0] == "general"
    assert _route(_arr(131_073, np.int64), C=10)[0] == "general_pipelined"  # the chunked route has no cap


def test_general_careful_replay():
    assert _route(_arr(99, np.float64), careful=True)[0] == "general"


def test_weights():
    x = _arr(99)
    assert _route(x, weights=[2, 3.5, np.float64(5)])[0] == "fused_one_call"
    assert _route(x, weights=[np.ones(99)] * 3)[0] == "general"  # np.float64 array weights
    # weights whose value float32 cannot hold: float64 arithmetic, the general shape
    route, call = _route(x, weights=[np.float64(1e40)] * 3)
    assert call.cts == {F64} and route == "general_one_call"
    route, call = _route(x, weights=[np.float64(1e40), 1.0, 2.0])
    assert call.cts == {F32, F64} and route == "general"
    # a python float of that size widens under numpy 1's value-based casting
    # and stays float32 (overflowing) under numpy 2's: the route follows
    # payload.compute_dtype either way
    with np.errstate(over="ignore", invalid="ignore"):
        ct = compute_dtype(F32, 1e40, 18)
        route, call = _route(x, weights=[1e40] * 3)
    assert call.cts == {ct} and route == ("general_one_call" if ct == F64 else "fused_one_call")
    # layers of two dtypes under scalar weights: the general path groups them layer by layer
    assert _route([x, _arr(7, np.float64)], weights=[1, 2, 3])[0] == "general"
    assert _route([x, _arr(7)], weights=[np.ones(1)] * 3)[0] == "general"  # array weights are never host-packed


def test_host_packed():
    """More than one host layer, each party's layers of one dtype, outside
    the one-call and chunked shapes."""
    two = [_arr(15), _arr(7)]
    assert _route(two, fused=False)[0] == "general_host_packed"
    assert _route(two, keep_masked=True)[0] == "general_host_packed"


def test_everything_else_is_general():
    import torch

    x = _arr(99)
    assert _route(x, keep_masked=True)[0] == "general"
    assert _route(x, fused=False)[0] == "general"
    assert _route(x, gpus=[0, 0, 1])[0] == "general"
    assert _route(torch.zeros(99))[0] == "general"
    assert _route([torch.zeros(15), torch.zeros(7)])[0] == "general"
    assert _route(_arr(0))[0] == "general"
    assert _route(x, C=1)[0] == "general"
