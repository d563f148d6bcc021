"""Error paths of the blocking host-array entries (include/sfl_sa.h:
sa_fused_clients_host_f32, sa_clients_host, sa_mask_host,
sa_sum_decode_host).

Each entry enqueues its host-to-device copy before the launch function that
validates ``fxp_bits`` runs, so a call with ``fxp_bits = 63`` fails AFTER
work that reads the caller's pinned scratch is on the stream.  The contract
(sa_host_calls.hip, the comment above ``drain``): an error returned after the first
copy was enqueued leaves the stream drained, so the caller may reuse or free
the scratch at once.  Checked here directly -- the stream is idle the moment
the failing call returns -- and functionally: the pinned scratch is
scribbled over right away and the very same scratch then serves a good call
whose outputs must be bit-exact against the oracle.

Below the error paths: the four entries at the edges of their scratch layout
(sa_host_layout.h: n around the n_pad rounding, odd and largest client
counts, both sides of sa_clients_host's zero-by-copy threshold), bit-exact
and with guard bytes behind the advertised scratch sizes left untouched; and
the server sums' chained launches (more than 32 inputs) and sa_sum_u64 with
``out`` aliasing its first input.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gpu_copies import DEV, _dev, _host, _item  # noqa: E402
from oracle import secagg as o  # noqa: E402

pytestmark = pytest.mark.gpu
N = 2_000_003  # ~8-16 MB per copy: a copy still in flight at return would be seen by query()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sfl_amd import _lib as L

    L.lib()


def _inputs(c, n=N, dtype=np.float32):
    rng = np.random.default_rng(1000 + c)
    x = rng.standard_normal(n) * 3
    return x.astype(np.int64) if dtype == np.int64 else x.astype(dtype)


def _scratch(pin_bytes, dev_bytes):
    pinned = torch.empty(pin_bytes, dtype=torch.uint8).pin_memory()
    dev = torch.empty(dev_bytes, dtype=torch.uint8, device=DEV)
    return pinned, dev


def _streams_for(c, names, offset=0):
    """client c's streams in its masker's order (peers by index), oracle seeds"""
    from sfl_amd import _lib as L

    out = []
    for j in range(len(names)):
        if j == c:
            continue
        seed = o.pair_seed(min(c, j), max(c, j))
        out.append((L.pcg64_advance(L.pcg64_from_seed(seed), offset), 1 if j > c else -1, j))
    return out


def _oracle_masked(x, c, names, offset=0, weight=None):
    q = o.quantize(x, weight)
    seeds = {names[j]: o.pair_seed(min(c, j), max(c, j)) for j in range(len(names)) if j != c}
    return o.mask_client(q, names[c], seeds, offset)


def _fail_then_idle(call):
    from sfl_amd import _lib as L

    torch.cuda.synchronize()
    with pytest.raises(L.SALibraryError, match="code -1"):
        call()
    # drained on return: nothing of the failed call is still reading the scratch
    assert torch.cuda.current_stream(DEV).query()


def test_mask_host_error_after_copy_drains_then_reuse_is_exact():
    from sfl_amd import kernels as K

    names = ["a", "b", "c"]
    x = _inputs(0)
    pinned, dev = _scratch(*K.mask_host_scratch(N, 4))
    st = _streams_for(0, names, offset=12345)
    _fail_then_idle(lambda: K.mask_host(x, np.float32, st, pinned, dev, fxp_bits=63))
    pinned.fill_(0xA5)
    dev.fill_(0x5A)
    out, flags = K.mask_host(x, np.float32, st, pinned, dev)
    assert flags == 0
    assert np.array_equal(out, _oracle_masked(x, 0, names, offset=12345))


def test_sum_decode_host_error_after_copy_drains_then_reuse_is_exact():
    from sfl_amd import kernels as K

    names = ["a", "b", "c"]
    masked = [_oracle_masked(_inputs(c), c, names) for c in range(3)]
    pinned, dev = _scratch(*K.sum_decode_host_scratch(3, N))
    _fail_then_idle(lambda: K.sum_decode_host(masked, pinned, dev, fxp_bits=63))
    pinned.fill_(0xA5)
    out, dig = K.sum_decode_host(masked, pinned, dev, divisor=3.0)
    s = o.server_sum(masked)
    assert np.array_equal(out, o.decode(s, divisor=3.0))
    assert [int(d) for d in dig] == [o.digest(m) for m in masked]


@pytest.mark.parametrize("dtype", [np.float64, np.int64])
def test_clients_host_error_after_copy_drains_then_reuse_is_exact(dtype):
    from sfl_amd import kernels as K

    names = ["a", "b", "c", "d"]
    xs = [_inputs(c, dtype=dtype) for c in range(4)]
    streams = [_streams_for(c, names) for c in range(4)]
    w = [1.0] * 4
    pinned, dev = _scratch(*K.host_clients_scratch(4, N, 8))
    _fail_then_idle(lambda: K.clients_host(xs, dtype, w, streams, pinned, dev, fxp_bits=63))
    pinned.fill_(0xA5)
    dev.fill_(0x5A)  # the large-sum branch fills its sum on the device: stale bytes must not leak in
    out, dig, flags = K.clients_host(xs, dtype, w, streams, pinned, dev, divisor=4.0)
    masked = [_oracle_masked(xs[c], c, names) for c in range(4)]
    assert flags == 0
    assert [int(d) for d in dig] == [o.digest(m) for m in masked]
    assert np.array_equal(out, o.decode(o.server_sum(masked), divisor=4.0))


def test_fused_clients_host_f32_error_after_copy_drains_then_reuse_is_exact():
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    C = 4
    names = [f"p{c}" for c in range(C)]
    xs = [_inputs(c) for c in range(C)]
    gens, signs = [], []
    for u in range(C):
        for v in range(u + 1, C):
            gens.append(L.pcg64_from_seed(o.pair_seed(u, v)))
            signs.append(1)
    pinned, dev = _scratch(*K.host_fused_scratch(C, N))
    _fail_then_idle(lambda: K.fused_clients_host_f32(xs, [1.0] * C, gens, signs, pinned, dev, fxp_bits=63))
    pinned.fill_(0xA5)
    dev.fill_(0x5A)
    res = K.fused_clients_host_f32(xs, [1.0] * C, gens, signs, pinned, dev, divisor=float(C))
    assert res is not None
    out, dig, flags = res
    masked = [_oracle_masked(xs[c], c, names) for c in range(C)]
    assert flags == 0
    assert [int(d) for d in dig] == [o.digest(m) for m in masked]
    assert np.array_equal(out, o.decode(o.server_sum(masked), divisor=float(C)))


# ---------------------------------------------------------------------------
# the scratch layout's edges
# ---------------------------------------------------------------------------
GUARD = 64
EDGE_N = [1, 3, 4, 5]  # n_pad rounds 1, 3 and 5 up; 1, 3, 5 have the odd tail


def _guarded(pin_bytes, dev_bytes):
    """scratch of the advertised sizes + GUARD bytes each, all of it patterned"""
    pinned, dev = _scratch(pin_bytes + GUARD, dev_bytes + GUARD)
    pinned.fill_(0xA5)
    dev.fill_(0x5A)
    return pinned, dev


def _guards_untouched(pinned, dev, pin_bytes, dev_bytes):
    torch.cuda.synchronize()
    assert pinned.numel() == pin_bytes + GUARD and dev.numel() == dev_bytes + GUARD
    assert bool((pinned[pin_bytes:] == 0xA5).all()), "write past the advertised pinned scratch"
    assert bool((dev[dev_bytes:] == 0x5A).all()), "write past the advertised device scratch"


def _names(C):
    return [f"p{c:02d}" for c in range(C)]


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mask_host_at_layout_edges(n, dtype):
    from sfl_amd import kernels as K

    names = _names(3)
    x = _inputs(0, n, dtype)
    sizes = K.mask_host_scratch(n, x.dtype.itemsize)
    pinned, dev = _guarded(*sizes)
    out, flags = K.mask_host(x, dtype, _streams_for(0, names, offset=7), pinned, dev)
    assert flags == 0
    assert np.array_equal(out, _oracle_masked(x, 0, names, offset=7))
    _guards_untouched(pinned, dev, *sizes)


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("C", [1, 2, 32])
def test_sum_decode_host_at_layout_edges(n, C):
    from sfl_amd import kernels as K

    names = _names(C)
    masked = [_oracle_masked(_inputs(c, n), c, names) for c in range(C)]
    sizes = K.sum_decode_host_scratch(C, n)
    pinned, dev = _guarded(*sizes)
    out, dig = K.sum_decode_host(masked, pinned, dev, divisor=float(C))
    assert np.array_equal(out, o.decode(o.server_sum(masked), divisor=float(C)))
    assert [int(d) for d in dig] == [o.digest(m) for m in masked]
    _guards_untouched(pinned, dev, *sizes)


def _clients_host_case(C, n, dtype):
    from sfl_amd import kernels as K

    names = _names(C)
    xs = [_inputs(c, n, dtype) for c in range(C)]
    streams = [_streams_for(c, names) for c in range(C)]
    sizes = K.host_clients_scratch(C, n, xs[0].dtype.itemsize)
    pinned, dev = _guarded(*sizes)
    out, dig, flags = K.clients_host(xs, dtype, [1.0] * C, streams, pinned, dev, divisor=float(C))
    masked = [_oracle_masked(xs[c], c, names) for c in range(C)]
    assert flags == 0
    assert [int(d) for d in dig] == [o.digest(m) for m in masked]
    assert np.array_equal(out, o.decode(o.server_sum(masked), divisor=float(C)))
    _guards_untouched(pinned, dev, *sizes)


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("C", [2, 3, 9])
def test_clients_host_at_layout_edges(n, C):
    _clients_host_case(C, n, np.float32)


@pytest.mark.parametrize("n", [2048, 2049])  # a 16 KiB sum rides the copy as zeros, a larger one is filled on the device
@pytest.mark.parametrize("dtype", [np.float64, np.int64])
def test_clients_host_both_sides_of_the_zero_by_copy_threshold(n, dtype):
    _clients_host_case(3, n, dtype)


@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("C", [2, 3, 8])
def test_fused_clients_host_f32_at_layout_edges(n, C):
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    names = _names(C)
    xs = [_inputs(c, n) for c in range(C)]
    gens = [L.pcg64_from_seed(o.pair_seed(u, v)) for u in range(C) for v in range(u + 1, C)]
    sizes = K.host_fused_scratch(C, n)
    pinned, dev = _guarded(*sizes)
    res = K.fused_clients_host_f32(xs, [1.0] * C, gens, [1] * len(gens), pinned, dev, divisor=float(C))
    assert res is not None
    out, dig, flags = res
    masked = [_oracle_masked(xs[c], c, names) for c in range(C)]
    assert flags == 0
    assert [int(d) for d in dig] == [o.digest(m) for m in masked]
    assert np.array_equal(out, o.decode(o.server_sum(masked), divisor=float(C)))
    _guards_untouched(pinned, dev, *sizes)


# ---------------------------------------------------------------------------
# the server sums' chained launches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 4099])
@pytest.mark.parametrize("k", [33, 70])  # two and three launches of up to 32 inputs
@pytest.mark.parametrize("shift", [0, 1])
def test_sum_f64_chain_adds_strictly_left_to_right(k, n, shift):
    """More than 32 inputs: later launches continue from ``out``.  float64
    addition in input order, 16-byte aligned (shift 0) and one element into
    the allocations (shift 1: the any-alignment kernel)."""
    from sfl_amd import kernels as K

    rng = np.random.default_rng(100 * k + n)
    ws = [rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4) for _ in range(k)]
    wb = []
    for w in ws:
        b = torch.empty(n + 1, dtype=torch.float64, device=DEV)
        b[shift:shift + n] = _dev(w)
        wb.append(b[shift:shift + n])
    ob = torch.full((n + 1,), float("nan"), dtype=torch.float64, device=DEV)
    got = K.sum_f64(wb, ob[shift:shift + n])
    torch.cuda.synchronize()
    assert np.array_equal(_host(got), functools.reduce(np.add, ws))
    assert np.isnan(_item(ob[n if shift == 0 else 0]))  # nothing written past the vector


@pytest.mark.parametrize("k", [2, 33])
def test_sum_u64_out_may_alias_its_first_input(k):
    from sfl_amd import kernels as K

    n = 4099
    rng = np.random.default_rng(k)
    host = [rng.integers(0, 2**64 - 1, n, dtype=np.uint64) for _ in range(k)]
    ins = [_dev(h.view(np.int64)) for h in host]
    got = K.sum_u64(ins, ins[0])
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(got), o.server_sum(host))
    for h, t in zip(host[1:], ins[1:]):
        assert np.array_equal(K.as_u64(t), h)  # the other inputs are only read
