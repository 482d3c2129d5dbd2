"""numpy restatement of dpc_knn_batched, dpc_pca_normals and the normal-consistency metric (include/dpc_render.h).

    knn                  the full d2 matrix in the compute type, with the header's expression, and a stable argsort
    pca_normals          two-pass covariance of the valid neighbours in fp64, np.linalg.eigh, the two sign rules
    nearest              dpc_nearest_batched's neighbour: the first minimum of sqrt(d2) in the compute type
    normal_consistency   (a, b, (a + b) / 2) of one prediction against one GT cloud
    sphere, box, torus   the noisy test shapes
"""
import numpy as np

STATUS_BAD_INDEX, STATUS_NONFINITE = 1, 8
EPS = 2.0 ** -52
MIN_GAP = 1e-3   # (l1 - l0) / trace below which a normal is left out of the angle check


# the shapes of the fixture's PCA cases (and of tools/bench_normals.py): noisy samples of a sphere, a box and a torus
def sphere(rng, n):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return 0.4 * v * (1.0 + 0.01 * rng.normal(size=(n, 1)))


def box(rng, n):
    p = rng.uniform(-0.5, 0.5, size=(n, 3)) * np.array([0.8, 0.6, 0.4])
    face = rng.integers(0, 6, size=n)
    half = np.array([0.4, 0.3, 0.2])
    p[np.arange(n), face % 3] = np.where(face < 3, 1.0, -1.0) * half[face % 3]
    return p + 0.002 * rng.normal(size=(n, 3))


def torus(rng, n):
    u, v = rng.uniform(0, 2 * np.pi, size=n), rng.uniform(0, 2 * np.pi, size=n)
    r = 0.12 + 0.002 * rng.normal(size=n)
    return np.stack([(0.3 + r * np.cos(v)) * np.cos(u), (0.3 + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)


def d2_matrix(q, r, dtype):
    """[len(q), len(r)] squared distances in dtype: d = ref - q; (d0*d0 + d1*d1) + d2*d2, nothing fused."""
    q, r = np.asarray(q, dtype=dtype).reshape(-1, 3), np.asarray(r, dtype=dtype).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        d = r[None, :, :] - q[:, None, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn(q, r, k, dtype=np.float32):
    """(idx [Q,k] int32, d2 [Q,k] dtype, status): the k references smallest by (d2, j), ascending; a NaN d2 is no
    candidate (status NONFINITE); slots without a candidate hold -1 and +inf."""
    m = d2_matrix(q, r, dtype)
    Q, R = m.shape
    idx = np.full((Q, k), -1, dtype=np.int32)
    d2 = np.full((Q, k), np.inf, dtype=dtype)
    if R:
        order = np.argsort(m, axis=1, kind="stable")[:, :k]   # NaN sorts behind +inf
        vals = np.take_along_axis(m, order, axis=1)
        ok = ~np.isnan(vals)
        w = order.shape[1]
        idx[:, :w] = np.where(ok, order, -1)
        d2[:, :w] = np.where(ok, vals, np.inf)
    return idx, d2, (STATUS_NONFINITE if np.isnan(m).any() else 0)


def knn_brute(q, r, k, dtype=np.float32):
    """The same by a loop over queries and an explicit sort of (d2, j) pairs: the check of knn on a tiny case."""
    q, r = np.asarray(q, dtype=dtype).reshape(-1, 3), np.asarray(r, dtype=dtype).reshape(-1, 3)
    idx, d2 = [], []
    for p in q:
        cand = []
        for j, x in enumerate(r):
            d = x - p
            v = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if not np.isnan(v):
                cand.append((v, j))
        cand.sort()
        cand = cand[:k] + [(dtype(np.inf), -1)] * (k - min(k, len(cand)))
        idx.append([j for _, j in cand])
        d2.append([v for v, _ in cand])
    return np.asarray(idx, dtype=np.int32).reshape(len(q), k), np.asarray(d2, dtype=dtype).reshape(len(q), k)


def covariance(r, idx):
    """(C [Q,3,3], c [Q], status) of the valid slots of idx [Q,k] into r, in fp64, from the deviations."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < len(r))
    status = STATUS_BAD_INDEX if (~ok & (idx != -1)).any() else 0
    c = ok.sum(axis=1)
    x = np.where(ok[..., None], r[np.where(ok, idx, 0)] if len(r) else 0.0, 0.0)
    cn = np.maximum(c, 1).astype(np.float64)[:, None]
    mu = x.sum(axis=1) / cn
    dev = np.where(ok[..., None], x - mu[:, None, :], 0.0)
    C = np.einsum("qki,qkj->qij", dev, dev) / cn[:, :, None]
    return C, c, status


def orient(n, q=None, viewpoint=None):
    """The sign rules on normals n [Q,3]: towards viewpoint (n . (viewpoint - q) >= 0), or the component of largest
    magnitude positive (the lowest axis on equal magnitudes)."""
    n = np.array(n, dtype=np.float64)
    if viewpoint is not None:
        flip = np.einsum("qi,qi->q", n, np.asarray(viewpoint, dtype=np.float64)[None, :] - np.asarray(q, dtype=np.float64)) < 0
    else:
        a = np.argmax(np.abs(n), axis=1)   # the first of equal maxima
        flip = n[np.arange(len(n)), a] < 0
    n[flip] = -n[flip]
    return n


def pca_normals(q, r, idx, viewpoint=None):
    """(normals [Q,3], eigenvalues [Q,3] ascending, status) as dpc_pca_normals defines them, through np.linalg.eigh."""
    C, c, status = covariance(r, idx)
    w, v = np.linalg.eigh(C)
    n = orient(v[:, :, 0], np.asarray(q, dtype=np.float64).reshape(-1, 3), viewpoint)
    n[c < 3] = 0.0
    return n, np.maximum(w, 0.0), status


def unit(evals):
    """2^-52 trace / (l1 - l0) per query (inf where l1 == l0), and the relative gap (l1 - l0) / trace."""
    evals = np.asarray(evals, dtype=np.float64)
    tr = evals.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(tr > 0, (evals[:, 1] - evals[:, 0]) / tr, 0.0)
        return np.where(gap > 0, EPS / gap, np.inf), gap


def sin_angle(a, b):
    """|a x b| / (|a| |b|) per row: the sine of the angle between the lines of a and b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def estimate_normals(cloud, k, viewpoint=None):
    """Normals and eigenvalues of a cloud searched against itself, in the cloud's own precision."""
    cloud = np.asarray(cloud)
    idx, _, _ = knn(cloud, cloud, k, np.float64 if cloud.dtype == np.float64 else np.float32)
    n, w, _ = pca_normals(cloud, cloud, idx, viewpoint)
    return n, w


def nearest(src, tgt, dtype):
    """The index dpc_nearest_batched reports: the first minimum of sqrt(d2) in dtype."""
    return np.argmin(np.sqrt(d2_matrix(src, tgt, dtype)), axis=1)


def normal_consistency(pred, gt, n_pred, n_gt):
    """(a, b, (a + b) / 2): a = mean over the prediction's points of |Np . Ng[nearest GT point]|, b the same from the GT
    side; fp64 when either cloud is, as chamfer_batched.  An empty prediction gives NaN for a."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    dtype = np.float64 if np.float64 in (pred.dtype, gt.dtype) else np.float32
    n_pred, n_gt = np.asarray(n_pred, dtype=np.float64), np.asarray(n_gt, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if len(pred):
            a = np.mean(np.abs(np.einsum("qi,qi->q", n_pred, n_gt[nearest(pred, gt, dtype)])))
            b = np.mean(np.abs(np.einsum("qi,qi->q", n_gt, n_pred[nearest(gt, pred, dtype)])))
        else:
            a = b = np.float64(np.nan)
    return np.array([a, b, (a + b) / 2.0])
