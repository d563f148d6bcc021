"""The masking kernel's kernel-argument layout (sa_internal.h: the streams'
constants by draw group, two 16-dword scalar loads per group and tile; the
clients' input pointers and accumulator start values as arrays; the sign
masks as 64-bit compare operands with the negated clients' flip folded in by
the launcher), bit-exact against oracle/secagg.py on every shape that shares
it:

* the fused shapes (L local clients, X cross streams each) of 8 clients over
  1, 2, 4 and 8 ranks: (8, 0), (4, 4), (2, 6), (1, 7) -- sum-only, and with
  digests plus every client's masked vector;
* one multi-launch shape (32 clients over 8 ranks: a fused first launch and
  masks-only launches of the remaining cross streams);
* the general single-client path in continue mode (20 streams: a first pass
  and a continuing pass, and a pass continuing from a caller's vector).

Lengths: 1, 511, 513 (one lane, one element short of / past a 512-element
tile) and one length just over two sweeps of the launch's grid with an odd
tail, so the merged tile jump, the second sweep and the bounds-checked tail
all run in one launch: 600,001 for L = 8 (2 blocks per CU x 256 CUs x 512
elements = 262,144 per sweep), 2,000,001 for one client with 7 streams (7
blocks per CU: 917,504 per sweep), and between them for (4, 4), (2, 6) and
the masks-only launches (3 to 5 blocks per CU).

Client names are not in sorted order, so both mask signs occur among the
internal pairs and among the cross streams, and the negated clients (the
upper half of a launch's clients) carry cross streams of both signs: the
tests assert that.  The oracle's vectors are computed once per shape and
length and shared."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from gpu_copies import DEV, _dev, _item  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = (1, 511, 513)
# (clients, ranks, rank under test, the long length)
FUSED = {(8, 0): (8, 1, 0, 600_001), (4, 4): (8, 2, 1, 800_001), (2, 6): (8, 4, 2, 1_400_001),
         (1, 7): (8, 8, 5, 2_000_001)}
OFFSET = 1000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _names(C):
    """C distinct names whose order is not the clients' order."""
    return [f"party{(5 * c + 3) % C:02d}" for c in range(C)] if C % 5 else [f"party{(3 * c + 1) % C:02d}" for c in range(C)]


@functools.lru_cache(maxsize=None)
def _reference(C, W, rank, n):
    """(plan, names, seeds, inputs, the local clients' masked vectors) -- read-only."""
    from oracle import secagg as o
    from sfl_amd.parallel_sum import plan_rank

    names = _names(C)
    assert len(set(names)) == C and names != sorted(names)
    seeds = o.seeds_for(names)
    plan = plan_rank(names, W, rank)
    rng = np.random.default_rng(1000 * C + 10 * W + rank + n)
    xs = [(rng.standard_normal(n) * 1e-2).astype(np.float32) for _ in plan.clients]
    masked = [o.mask_client(o.quantize(x), names[c], seeds[names[c]], OFFSET) for x, c in zip(xs, plan.clients)]
    for a in xs + masked:
        a.setflags(write=False)
    return plan, names, seeds, xs, masked


def _assert_signs(plan):
    """Both signs among the pairs and the cross streams; for a launch with
    negated clients and cross streams, both signs on the negated clients."""
    Lc = len(plan.clients)
    if plan.pair_signs:
        assert {1, -1} <= set(plan.pair_signs) or Lc == 2
    if plan.cross:
        assert {1, -1} == {s for _, _, s in plan.cross}
    if Lc >= 2 and plan.cross:
        upper = set(plan.clients[Lc // 2:])
        assert {1, -1} == {s for c, _, s in plan.cross if c in upper}, "flipped cross streams of both signs"


def _run_fused(C, W, rank, n, full):
    from oracle import secagg as o
    from sfl_amd import kernels as K
    from sfl_amd.parallel_sum import plan_generators

    plan, names, seeds, xs, masked = _reference(C, W, rank, n)
    _assert_signs(plan)
    Lc = len(plan.clients)
    pg, ps, cross = plan_generators(plan, lambda u, v: seeds[names[u]][names[v]], offset=OFFSET)
    s = torch.empty(n, dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    dig = torch.zeros(Lc, dtype=torch.int64, device=DEV) if full else None
    mo = [torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(Lc)] if full else None
    K.fused_clients([_dev(x.copy()) for x in xs], [1.0] * Lc, pg, ps, cross, plan.n_cross, s,
                    digests=dig, flags=flags, masked_outs=mo)
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(s), o.server_sum(masked)), "masked sum"
    assert int(_item(flags)) == 0, "reject flag"
    if full:
        for c in range(Lc):
            assert np.array_equal(K.as_u64(mo[c]), masked[c]), f"masked vector of local client {c}"
        assert [int(v) for v in K.as_u64(dig)] == [o.digest(m) for m in masked], "digests"


@pytest.mark.parametrize("full", [False, True], ids=["sum_only", "digests_and_vectors"])
@pytest.mark.parametrize("shape", sorted(FUSED), ids=lambda s: f"L{s[0]}X{s[1]}")
@pytest.mark.parametrize("length", SMALL + ("sweeps",))
def test_fused_shapes_equal_oracle(shape, length, full):
    C, W, rank, long_n = FUSED[shape]
    plan = _reference(C, W, rank, 1)[0]
    assert (len(plan.clients), plan.n_cross) == shape
    _run_fused(C, W, rank, long_n if length == "sweeps" else length, full)


def test_both_signs_and_flipped_cross_streams_occur():
    """What the shapes above are chosen for: pair streams and cross streams of
    both signs, and cross streams of both signs on clients the kernel keeps
    negated (the upper half of (4, 4) and (2, 6))."""
    seen_pairs, seen_flipped = set(), set()
    for (L, X), (C, W, rank, _) in FUSED.items():
        plan = _reference(C, W, rank, 1)[0]
        _assert_signs(plan)
        seen_pairs |= set(plan.pair_signs)
        if L >= 2 and X:
            seen_flipped |= {s for c, _, s in plan.cross if c in plan.clients[L // 2:]}
    assert seen_pairs == {1, -1} and seen_flipped == {1, -1}


@pytest.mark.parametrize("n", SMALL + (800_001,))
def test_multi_launch_with_masks_only_tail_equals_oracle(n):
    """32 clients over 8 ranks: 4 local clients, 6 pairs + 4 x 28 cross
    streams -- one fused sum-only launch and masks-only launches adding the
    remaining cross streams into the sum."""
    C, W, rank = 32, 8, 3
    plan = _reference(C, W, rank, n)[0]
    assert len(plan.pairs) + len(plan.cross) > 32  # beyond one launch
    _run_fused(C, W, rank, n, full=False)


@pytest.mark.parametrize("n", SMALL + (2_000_001,))
def test_single_client_continue_mode_equals_oracle(n):
    """sa_mask with 20 streams: 16 in the first pass, 4 in a pass that
    continues from the masked vector (the general single-client kernel); then
    the same 20 streams continuing from a caller's quantized vector (x = None)."""
    from oracle import secagg as o
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K

    names = _names(21)
    me = names[7]
    seeds = o.seeds_for(names)[me]
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    q = o.quantize(x)
    exp = o.mask_client(q, me, seeds, OFFSET)
    streams = [(L.pcg64_advance(L.pcg64_from_seed(seeds[p]), OFFSET), 1 if p > me else -1, i)
               for i, p in enumerate(names) if p != me]
    assert len(streams) == 20 and {1, -1} == {s for _, s, _ in streams}
    out = torch.empty(n, dtype=torch.int64, device=DEV)
    acc = torch.zeros(n, dtype=torch.int64, device=DEV)
    dig = torch.zeros(1, dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.mask(_dev(x), out, streams, sum_accum=acc, digest=dig, flags=flags)
    prior = _dev(q.view(np.int64))
    K.mask(None, prior, streams, flags=flags)
    torch.cuda.synchronize()
    assert np.array_equal(K.as_u64(out), exp), "masked vector"
    assert np.array_equal(K.as_u64(acc), exp), "sum accumulator"
    assert int(K.as_u64(dig)[0]) == o.digest(exp), "digest"
    assert np.array_equal(K.as_u64(prior), exp), "continued from the caller's vector"
    assert int(_item(flags)) == 0, "reject flag"


def test_zero_draw_in_a_group_raises_the_reject_flag():
    """A raw draw of 0 in the last pair stream of the 8-client launch (its
    last element, in the bounds-checked tail) sets the flag; the same stream
    one draw further on does not."""
    from sfl_amd import _lib as L
    from sfl_amd import kernels as K
    from sfl_amd.parallel_sum import plan_generators
    from test_gpu_rejection import forced_zero_state

    C, W, rank, n = 8, 1, 0, 513
    plan, names, seeds, xs, _ = _reference(C, W, rank, n)
    pg, ps, cross = plan_generators(plan, lambda u, v: seeds[names[u]][names[v]], offset=OFFSET)
    got = []
    for k in (n - 1, n):  # the zero at the last element / just past the end
        bad = list(pg)
        bad[-1] = L.PCG64.of(*forced_zero_state(k))
        s = torch.empty(n, dtype=torch.int64, device=DEV)
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        K.fused_clients([_dev(x.copy()) for x in xs], [1.0] * C, bad, ps, cross, 0, s, flags=flags)
        torch.cuda.synchronize()
        got.append(int(_item(flags)) & L.SA_FLAG_PRG_REJECT)
    assert got == [L.SA_FLAG_PRG_REJECT, 0]
