"""FedSMP on the host: the keyed mask against a numpy restatement on
oracle.dp's Philox, the worker's step by hand, and the step against the
literal float64 chain of the reference."""
import numpy as np
import pytest

import smp_oracle as so
from sfl_amd import _lib as L
from sfl_amd.security.privacy import SMPMask, smp_step
from sfl_amd.security.privacy.smp import mask_key

KEYS = (0x0123456789ABCDEF, 0xF00DFACE0BADBEEF)
RATIOS = (0.0, 2.0**-32, 0.001, 0.1, 0.5, 0.8, 1 - 2.0**-33, 1.0)
U = 2.0**-24  # float32 unit roundoff


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("p", RATIOS)
@pytest.mark.parametrize("counter0", [0, 4, 4096, 2**34 + 4])
def test_mask_equals_the_numpy_restatement(p, counter0):
    m = SMPMask(KEYS[0], p)
    assert m.threshold == so.threshold(p) and m.divisor == so.divisor(p)
    for n in (0, 1, 3, 4, 5, 1025):
        got = L.smp_mask_host(m.layer(counter0), n)
        assert got.dtype == np.uint8 and got.shape == (n,)
        assert np.array_equal(got.astype(bool), so.kept(KEYS[0], p, counter0, n)), n
    if p == 1.0:
        assert L.smp_mask_host(m.layer(counter0), 1025).all()
    if p == 0.0:
        assert not L.smp_mask_host(m.layer(counter0), 1025).any()


def test_thresholds_at_the_edges():
    assert [so.threshold(p) for p in (0.0, 2.0**-32, 1 - 2.0**-33, 1.0)] == [0, 1, 2**32 - 1, 2**32]
    assert SMPMask(1, 1 - 2.0**-33).threshold == 2**32 - 1 and SMPMask(1, 2.0**-32).threshold == 1
    with pytest.raises(ValueError):
        SMPMask(1, 1.5)
    with pytest.raises(ValueError):
        SMPMask(1, -0.1)


def test_a_prefix_and_a_later_layer_see_the_same_stream():
    m = SMPMask(KEYS[1], 0.5)
    whole = L.smp_mask_host(m.layer(0), 4096 + 37)
    assert np.array_equal(L.smp_mask_host(m.layer(0), 100), whole[:100])
    assert np.array_equal(L.smp_mask_host(m.layer(4096), 37), whole[4096:])


@pytest.mark.parametrize("p", [0.1, 0.5, 0.8])
def test_mask_and_noise_domains_differ(p):
    """The same key in both roles: the mask is not `w < T` on the noise's words."""
    n = 4096
    got = L.smp_mask_host(SMPMask(KEYS[0], p).layer(0), n).astype(bool)
    noise_side = so.kept(KEYS[0], p, 0, n, domain=0)
    assert not np.array_equal(got, noise_side)
    # independent streams agree where two Bernoulli(p) draws do: p^2 + (1 - p)^2 of the time
    agree, want = np.mean(got == noise_side), p * p + (1 - p) * (1 - p)
    assert abs(agree - want) < 4 * np.sqrt(want * (1 - want) / n)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("p", [0.001, 0.1, 0.5, 0.8])
def test_kept_count_is_binomial(key, p):
    n = 2**20
    count = int(L.smp_mask_host(SMPMask(key, p).layer(0), n).sum(dtype=np.int64))
    pt = so.threshold(p) / 2**32  # the probability the threshold realises
    z = (count - pt * n) / np.sqrt(n * pt * (1 - pt))
    print(f"key {key:#x} p {p}: kept {count}, {z:+.2f} sd")
    assert abs(z) < 4


def _layers(seed=3):
    """Four entries: float32 (10), int64 (3), an empty float32 layer, float32 (2 x 7); a dropped
    -0.0, a dropped inf and a dropped NaN in the first."""
    rng = np.random.default_rng(seed)
    old = [rng.standard_normal(10).astype(np.float32), np.array([5, 6, 7], dtype=np.int64),
           np.zeros((0, 4), dtype=np.float32), rng.standard_normal((2, 7)).astype(np.float32)]
    new = [old[0] + rng.standard_normal(10).astype(np.float32) * np.float32(0.1), np.array([6, 7, 8], dtype=np.int64),
           np.zeros((0, 4), dtype=np.float32), old[3] + rng.standard_normal((2, 7)).astype(np.float32) * np.float32(0.1)]
    return old, new


def test_host_step_by_hand():
    key, p = KEYS[0], 0.5
    old, new = _layers()
    m0 = so.kept(key, p, 0, 10)
    dropped = np.flatnonzero(~m0)
    assert dropped.size >= 3 and m0.any()
    old[0][dropped[0]], old[0][dropped[1]], old[0][dropped[2]] = np.float32(-0.0), np.float32(np.inf), np.float32(np.nan)
    new[0][dropped[1]] = np.float32(np.inf)  # inf - inf under a dropped position
    got = smp_step(old, new, SMPMask(key, p))
    c = np.float32(p + 1e-6)
    # the counters: 10 elements take 12 indices, the int64 entry and the empty layer none
    masks = [m0, None, np.zeros((0, 4), bool), so.kept(key, p, 12, 14).reshape(2, 7)]
    for li in (0, 2, 3):
        assert got[li].dtype == np.float32 and got[li].shape == old[li].shape
        with np.errstate(all="ignore"):
            want = np.where(masks[li], old[li] + (new[li] - old[li]) / c, old[li])
        assert np.array_equal(_bits(got[li]), _bits(want)), li
        assert np.array_equal(_bits(got[li])[~masks[li]], _bits(old[li])[~masks[li]]), li  # w0's bits
    assert _bits(got[0])[dropped[0]] == 0x80000000 and np.isinf(got[0][dropped[1]])
    assert got[1] is new[1]  # the trained value, untouched
    by_hand = so.step(old, new, key, p)
    assert all(np.array_equal(_bits(got[li]), _bits(by_hand[li])) for li in (0, 2, 3))


def test_host_step_with_a_model_gdp_and_other_dtypes():
    key, p = KEYS[1], 0.8
    old, new = _layers(seed=5)
    gdp = so.clip_only(0.05)
    got = smp_step(old, new, SMPMask(key, p), gdp)
    want = so.step(old, new, key, p, gdp)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # the clip was active, so the kept elements differ from the unclipped step's
    assert not np.array_equal(got[0], smp_step(old, new, SMPMask(key, p))[0])
    with pytest.raises(NotImplementedError, match="float32 models only"):
        smp_step([np.zeros(4)], [np.ones(4)], SMPMask(key, p))
    with pytest.raises(ValueError):
        smp_step(old, new[:2], SMPMask(key, p))


@pytest.mark.parametrize("clip,each_layer", [(None, False), (0.05, False), (0.05, True), (1e3, False), (1e3, True)],
                         ids=["no_dp", "clipping", "clipping_each_layer", "clip_idle", "clip_idle_each_layer"])
@pytest.mark.parametrize("p", [0.1, 0.8, 1.0])
def test_host_step_against_the_literal_reference(p, clip, each_layer):
    """The reference's chain (FedSMP_torch.py:105-119) runs in float64 because its mask is int64;
    the host form rounds to float32 after every operation.  With u = 2^-24 and t the reference's
    clipped, scaled update of a kept element:

    * d: the subtraction, c = float32(p + 1e-6) and the division round once each, so d is off
      by at most 3 u |d| (to first order);
    * the norm: every d is within 3 u, so is the true norm of the float32 d; the float32 dot
      rounds once (u, halved by the square root) and the float32 square root once: 4.5 u against
      the reference's float64 norm, for one layer and, the squares being added in float64, for
      the sum over the layers and for sqrt(layer * all);
    * the scale min(1, clip / norm) inherits the 4.5 u and rounds to float32: 5.5 u;
    * the product d * scale rounds once: 3 + 5.5 + 1 = 9.5 u |t|; the noise is 0 and adds nothing;
    * the sum w0 + t rounds once: u |w0 + t| <= u (|w0| + |t|).

    Together |host - reference| <= u (|w0| + 10.5 |t|) to first order; the second-order terms
    (about 50 u^2 |t|) and the reference's own float64 roundings (a few 2^-53) are far below the
    0.5 u |t| by which the asserted bound u (|w0| + 11 |t|) exceeds that.  A dropped element is
    w0 on both sides."""
    key = KEYS[0]
    rng = np.random.default_rng(11)
    old = [rng.standard_normal(s).astype(np.float32) for s in ((64, 33), (50,), (3, 3, 5, 5))]
    new = [o + (rng.standard_normal(o.shape) * 0.05).astype(np.float32) for o in old]
    ref = so.reference_f64(old, new, key, p, clip, each_layer)
    got = smp_step(old, new, SMPMask(key, p), None if clip is None else so.clip_only(clip, each_layer))
    worst = 0.0
    for o, r, g, m in zip(old, ref, got, so.masks(key, p, old)):
        assert r.dtype == np.float64 and g.dtype == np.float32
        t = np.abs(r - o.astype(np.float64))
        bound = U * (np.abs(o).astype(np.float64) + 11 * t)
        err = np.abs(g.astype(np.float64) - r)
        assert np.array_equal(g[~m], o[~m]) and np.array_equal(r[~m], o[~m].astype(np.float64))
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound)
    print(f"p {p} clip {clip} each_layer {each_layer}: worst error / bound {worst:.3f}")
    if clip == 0.05:  # the clip did something
        unclipped = so.reference_f64(old, new, key, p, None)
        assert not np.allclose(ref[0], unclipped[0], rtol=1e-3, atol=0)


def test_mask_key_sequence():
    assert mask_key(7, 0) == mask_key(7, 0) != mask_key(7, 1) != mask_key(8, 1)
    import hashlib

    want = hashlib.sha256(b"sfl_amd.fed_smp.mask" + (7).to_bytes(8, "little") + (3).to_bytes(8, "little")).digest()
    assert mask_key(7, 3) == int.from_bytes(want[:8], "little")
    assert 0 <= mask_key(None, 0) < 2**64 and mask_key(None, 0) != mask_key(None, 0)
