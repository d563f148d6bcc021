"""The reference's MARS arithmetic restated for the tests (agg_mars.py's
``CLP`` and decision functions, in the uploads' own float type: the float32
scale multiplied into the float32 weights before LAPACK's SVD), and the
planted six-client model both test files use."""
import numpy as np
from scipy.stats import wasserstein_distance
from sklearn.cluster import KMeans

SHAPES = [(8, 3, 3, 3), (8,), (8,), (8,), (8,), (16, 8, 3, 3), (16,), (16,), (16,), (16,), (10, 64)]
LABELS = [-1, 0, -1, -1, 0, -1]


def planted(T, seed=0, extra=()):
    """conv + BN + conv + BN + fc (then the layers of ``extra`` shapes); clients
    1 and 4 have a few channels scaled up by 4 to 8."""
    rng, more = np.random.default_rng(seed), np.random.default_rng(seed + 1000)  # (the same model with any extra)
    data = []
    for i in range(6):
        d = [(rng.standard_normal(s) * (0.01 if len(s) == 2 else 0.1)).astype(T) if len(s) != 1
             else (rng.uniform(0.5, 1.5, s) * 0.1).astype(T) for s in SHAPES]
        for var in (4, 9):
            d[var] = (d[var] * 10).astype(T)
        if i in (1, 4):
            d[0][:2] *= T(rng.uniform(4, 8))
            d[5][:3] *= T(rng.uniform(4, 8))
        data.append(d + [(more.standard_normal(s) * 0.01).astype(T) for s in extra])
    return data


def _top(values):
    values = np.asarray(values)
    return [v for v in values if v >= np.quantile(values, 0.95)]


def clp(params):
    kinds, at = [], 0
    while at < len(params):
        nd = params[at].ndim
        if nd == 1 and at + 3 < len(params) and all(q.ndim == 1 for q in params[at:at + 4]):
            kinds.append(("bn", at))
            at += 4
            continue
        if nd in (2, 4):
            kinds.append(("conv" if nd == 4 else "fc", at))
        at += 1
    out = []
    for n, (kind, at) in enumerate(kinds):
        w = params[at]
        if kind == "bn":
            out += _top(np.abs(w / np.sqrt(np.maximum(params[at + 3], 0) + 1e-5)))
        elif kind == "fc":
            out += _top([np.linalg.svd(w.reshape(len(w), -1), compute_uv=False)[0]])
        else:
            bn = kinds[n + 1][1] if n + 1 < len(kinds) and kinds[n + 1][0] == "bn" else None
            lips = []
            for ch in range(len(w)):
                m = w[ch].reshape(w.shape[1], -1)
                if bn is not None and ch < len(params[bn]):
                    m = m * np.abs(params[bn][ch] / np.sqrt(np.maximum(params[bn + 3][ch], 0) + 1e-5))
                lips.append(np.linalg.svd(m, compute_uv=False)[0])
            out += _top(lips)
    return np.array(out) if out else np.array([np.linalg.norm(q.ravel()) for q in params])


def labels(vectors, threshold):
    hist = [np.histogram(v, bins=50, density=True)[0] for v in vectors]
    n = len(vectors)
    dist = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            dist[i][j] = dist[j][i] = wasserstein_distance(hist[i], hist[j])
    km = KMeans(n_clusters=2, random_state=42, n_init=10).fit(dist).labels_
    groups = [[v for v, k in zip(vectors, km) if k == c] for c in range(2)]
    centres = [np.histogram(np.concatenate(g), bins=50, density=True)[0] for g in groups if g]
    if len(centres) < 2 or wasserstein_distance(*centres) <= threshold:
        return [0] * n
    bad = np.argmax([np.abs(c).sum() for c in centres])
    return [-1 if k == bad else 0 for k in km]
