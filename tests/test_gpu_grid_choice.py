"""The masking launch with its grid taken from qualifying_grid and the
three-carry draw, bit-exact against oracle/secagg.py at the sizes where the
new code can go wrong.

The draw (sa_draw3.h) is exact only for a carry-free multiplier (pcg128.h),
so launch_clients moves the grid to the nearest one whose tile jump
A^(grid*512 - 1) qualifies.  A small vector can now get more blocks than
tiles (1 tile -> grid 2: one block runs no iteration; 6 or 7 tiles -> 8;
9 -> 11), a capped grid can shrink (cap 496 -> 495), and every tile after a
block's first is reached by the jump multiplier, so the sizes below also go
past twice each shape's grid.  Every stream is checked at every element
against numpy's PCG64 through the oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from gpu_copies import DEV, _dev, _item  # noqa: E402

pytestmark = pytest.mark.gpu
T = 512  # elements per tile
NAMES8 = ["p3", "p0", "p6", "p1", "p7", "p2", "p5", "p4"]  # mixed order: both pair signs occur
N8 = 300_001  # grid 512, 586 tiles: 74 blocks take the tile jump a second time
SIZES8 = [1, 511, 512, 6 * T + 5, 7 * T - 3, 9 * T, N8]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gens(names, seeds, offset=0):
    from sfl_amd import _lib as L

    pg, ps = [], []
    for u in range(len(names)):
        for v in range(u + 1, len(names)):
            pg.append(L.pcg64_advance(L.pcg64_from_seed(seeds[names[u]][names[v]]), offset))
            ps.append(1 if names[v] > names[u] else -1)
    return pg, ps


@pytest.fixture(scope="module")
def eight():
    """8 clients x N8 and their oracle vectors, computed once: a shorter n is
    the same streams' prefix (element i of a stream is its i-th draw)."""
    from oracle import secagg as o

    rng = np.random.default_rng(808)
    xs = [(rng.standard_normal(N8) * 1e-2).astype(np.float32) for _ in NAMES8]
    seeds = o.seeds_for(NAMES8)
    masked = o.secure_masked(xs, NAMES8, seeds=seeds)
    for m in masked:
        m.setflags(write=False)
    total = o.server_sum(masked)
    total.setflags(write=False)
    pg, ps = _gens(NAMES8, seeds)
    return {"xs": xs, "xt": [_dev(x) for x in xs], "masked": masked, "sum": total,
            "pg": pg, "ps": ps}


@pytest.mark.parametrize("n", SIZES8)
def test_eight_clients_sum_only(eight, n):
    from sfl_amd import kernels as K

    s = torch.empty(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.fused_clients([x[:n] for x in eight["xt"]], [1.0] * 8, eight["pg"], eight["ps"], [], 0, s, flags=flags)
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(s), eight["sum"][:n])
    assert int(_item(flags)) == 0


@pytest.mark.parametrize("n", SIZES8)
def test_eight_clients_with_masked_outputs(eight, n):
    from oracle import secagg as o
    from sfl_amd import kernels as K

    s = torch.empty(n, dtype=torch.int64, device=DEV)
    mo = [torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(8)]
    dig = torch.zeros(8, dtype=torch.int64, device=DEV)
    K.fused_clients([x[:n] for x in eight["xt"]], [1.0] * 8, eight["pg"], eight["ps"], [], 0, s, digests=dig,
                    masked_outs=mo)
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(s), eight["sum"][:n])
    for c in range(8):
        assert np.array_equal(K.as_u64(mo[c]), eight["masked"][c][:n]), c
    assert [int(v) for v in K.as_u64(dig)] == [o.digest(m[:n]) for m in eight["masked"]]


def test_eight_clients_under_a_masking_reserve(eight):
    """sa_set_masking_reserve(8) caps the headline grid at 496 blocks, which
    does not qualify: the launch runs on 495."""
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    s = torch.empty(N8, dtype=torch.int64, device=DEV)
    try:
        L.check(L.lib().sa_set_masking_reserve(8), "reserve")
        K.fused_clients(eight["xt"], [1.0] * 8, eight["pg"], eight["ps"], [], 0, s)
        torch.cuda.synchronize()
    finally:
        L.lib().sa_set_masking_reserve(0)
    assert np.array_equal(K.as_u64(s), eight["sum"])


def _rank_case(C, W, r, n, offset, seed):
    """Rank r's clients of C over W ranks: inputs, generators and the oracle's partial sum."""
    from oracle import secagg as o
    from sfl_amd.parallel_sum import plan_generators, plan_rank

    names = [f"c{i:02d}" for i in range(C)]
    seeds = o.seeds_for(names)
    plan = plan_rank(names, W, r)
    rng = np.random.default_rng(seed)
    xs = {c: (rng.standard_normal(n) * 1e-2).astype(np.float32) for c in plan.clients}
    pg, ps, cross = plan_generators(plan, lambda u, v: seeds[names[u]][names[v]], offset=offset)
    exp = np.zeros(n, dtype=np.uint64)
    for c in plan.clients:
        exp += o.mask_client(o.quantize(xs[c]), names[c], seeds[names[c]], offset)
    return plan, [_dev(xs[c]) for c in plan.clients], pg, ps, cross, exp


# per-rank shapes of 8 clients: <4,4> (W = 2), <2,6> (W = 4), the lean <1,7> (W = 8); the long sizes go past
# twice the shape's grid (<1,7>: 7 blocks per CU x 256 CUs x 512 elements)
@pytest.mark.parametrize("W,n", [(2, 7 * T - 3), (2, 1_200_001), (4, 7 * T - 3), (4, 1_200_001),
                                 (8, 7 * T - 3), (8, 2_000_003)])
def test_per_rank_shapes(W, n):
    from sfl_amd import kernels as K

    plan, xt, pg, ps, cross, exp = _rank_case(8, W, W // 2, n, offset=3, seed=W * 7 + n % 5)
    assert (len(plan.clients), plan.n_cross) == (8 // W, 8 - 8 // W)
    s = torch.empty(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.fused_clients(xt, [1.0] * len(xt), pg, ps, cross, plan.n_cross, s, flags=flags)
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(s), exp)
    assert int(_item(flags)) == 0


def test_multi_launch_schedule_stored_and_accumulated():
    """4 clients + 28 cross streams each: a fused launch and masks-only
    <1,32> launches adding into the sum, every one on a grid of its own."""
    from sfl_amd import kernels as K

    n = 200_003
    plan, xt, pg, ps, cross, exp = _rank_case(32, 8, 5, n, offset=11, seed=32)
    assert len(plan.pairs) + len(plan.cross) > 32
    s = torch.empty(n, dtype=torch.int64, device=DEV)
    K.fused_clients(xt, [1.0] * 4, pg, ps, cross, plan.n_cross, s)
    init = np.random.default_rng(5).integers(0, 2**63, n, dtype=np.int64)
    acc = _dev(init)
    K.fused_clients(xt, [1.0] * 4, pg, ps, cross, plan.n_cross, acc, accumulate=True)
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(s), exp)
    assert np.array_equal(K.as_u64(acc), exp + init.view(np.uint64))


def test_sixteen_colocated_clients_bipartite_blocks():
    """16 co-located clients: two groups of 8 and four sa_fused_bipartite
    blocks (masks only), all through launch_clients."""
    from oracle import secagg as o
    from sfl_amd import kernels as K

    C, n = 16, 100_003
    names = [f"q{(5 * i) % C:02d}" for i in range(C)]
    seeds = o.seeds_for(names)
    rng = np.random.default_rng(16)
    xs = [(rng.standard_normal(n) * 1e-2).astype(np.float32) for _ in range(C)]
    exp = o.server_sum(o.secure_masked(xs, names, seeds=seeds))
    pg, ps = _gens(names, seeds)
    s = torch.empty(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.fused_clients([_dev(x) for x in xs], [1.0] * C, pg, ps, [], 0, s, flags=flags)
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(s), exp)
    assert int(_item(flags)) == 0
