"""FedSMP restated in numpy for the tests, sharing no code with the package:
the keyed mask on oracle.dp's Philox, the worker's float32 chain by hand, and
the literal float64 chain of the reference
(examples/security/h_gia/FedSMP_defense/FedSMP_torch.py:105-119 with
sfl/security/privacy/mechanism/mechanism_fl.py:62-135 at noise 0)."""
import numpy as np

from oracle import dp as od


def threshold(p: float) -> int:
    return min(2**32, int(p * 4294967296))


def divisor(p: float) -> np.float32:
    return np.float32(p + 1e-6)


def words(key: int, counter0: int, n: int, domain: int = 1) -> np.ndarray:
    """The Philox words of stream indices counter0 .. counter0 + n - 1 (counter0 % 4 == 0) with
    ``domain`` in the counter's third word: 1 is the mask's, 0 the DP noise's."""
    assert counter0 % 4 == 0
    blk = np.arange(counter0 // 4, (counter0 + n + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((blk.size, 4), dtype=np.uint32)
    ctr[:, 0] = (blk & od.MASK32).astype(np.uint32)
    ctr[:, 1] = (blk >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = domain
    return od.philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32)).reshape(-1)[:n]


def kept(key: int, p: float, counter0: int, n: int, domain: int = 1) -> np.ndarray:
    return words(key, counter0, n, domain).astype(np.uint64) < np.uint64(threshold(p))


def counters(layers) -> list:
    """Stream index of each float32 layer's first element (None for the other entries)."""
    out, c = [], 0
    for a in layers:
        if a.dtype != np.float32:
            out.append(None)
            continue
        out.append(c)
        c += -(-a.size // 4) * 4
    return out


def masks(key: int, p: float, layers) -> list:
    return [None if c0 is None else kept(key, p, c0, a.size).reshape(a.shape)
            for a, c0 in zip(layers, counters(layers))]


def step(old, new, key: int, p: float, model_gdp=None) -> list:
    """The worker's upload by hand, float32, one rounding per operation."""
    c = divisor(p)
    ms = masks(key, p, old)
    f = [i for i, m in enumerate(ms) if m is not None]
    with np.errstate(all="ignore"):
        ds = [np.where(ms[i], (new[i] - old[i]) / c, np.float32(0)) for i in f]
        assert all(d.dtype == np.float32 for d in ds)
        ts = model_gdp(ds) if model_gdp is not None and ds else ds
        out = list(new)
        for i, t in zip(f, ts):
            out[i] = np.where(ms[i], old[i] + t, old[i])
    return out


def reference_f64(old, new, key: int, p: float, clip=None, each_layer=False) -> list:
    """FedSMP_torch.py:105-119 as written, on float32 weights with an int64 mask (which makes
    everything after it float64) and GaussianModelDP at noise_multiplier 0 when ``clip`` is given."""
    grad_mask = [m.astype(np.int64) for m in masks(key, p, old)]
    grads = [v2 - v1 for v1, v2 in zip(old, new)]
    grads = [v2 * v1 for v1, v2 in zip(grads, grad_mask)]
    grads = [v / (p + 1e-6) for v in grads]
    if clip is not None:  # mechanism_fl.py:71-84, :104-107, :132-135; the noise is 0
        norm = lambda xs: np.sqrt(sum([np.linalg.norm(i) ** 2 for i in xs]))  # noqa: E731
        norm_all = norm(grads)
        with np.errstate(all="ignore"):
            if each_layer:
                grads = [g * min(1, clip / np.sqrt(norm([g]) * norm_all)) for g in grads]
            else:
                scale = min(1, clip / norm_all)
                grads = [g * scale for g in grads]
    grads = [v2 * v1 for v1, v2 in zip(grads, grad_mask)]
    return [v1 + v2 for v1, v2 in zip(old, grads)]


def clip_only(clip: float, each_layer: bool = False, num_updates: float = 2.0):
    """A model_gdp for host tests: oracle.dp's float32 restatement of GaussianModelDP at noise 0."""
    return lambda xs: od.gaussian_model_dp(xs, 0.0, num_updates, clip, is_clip_each_layer=each_layer)
