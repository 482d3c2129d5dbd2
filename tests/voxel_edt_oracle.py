"""Numpy restatement of the voxel distance rules of include/dpc_render.h (dpc_voxel_edt): the squared Euclidean distance
transform of an occupancy grid, twice over -- brute force over the seed list (the definition itself) and an independent
separable integer version for dense grids -- the six-neighbour shell, the stats of a (field, grid) pair, the F-score
conventions, and the seeded grids the voxel distance tests and the fixture tests/golden/f34_voxel_edt.npz share.
Everything is an integer but the F-score's ratios: there is one right answer and no tolerance.

F-score conventions (those of fscore, dpc/render/pointmesh.py, restated): precision = within / n of the prediction's
voxels, recall the same of the ground truth's; an empty side has 0 / 0 = NaN; a non-empty side measured against an empty
one reaches nothing and scores 0; F = 2 P R / (P + R), 0 where P + R = 0 and NaN where either is NaN.  "within tau" is
sq <= floor(tau^2) with tau^2 evaluated in fp64, i.e. distance <= tau."""
import numpy as np

from voxels_oracle import digest, pack_bits  # noqa: F401

NONE = 2 ** 31 - 1
MAX_THRESHOLDS = 8
_INF = np.int64(1) << 40


def seeds_of(occ, of_clear=False):
    occ = np.asarray(occ, dtype=bool)
    return ~occ if of_clear else occ


def edt_brute(occ, of_clear=False):
    """int32 [D,H,W]: min over the seeds of (d-d')^2 + (h-h')^2 + (w-w')^2, NONE everywhere without a seed.  Every voxel
    against every seed, one d-plane at a time: [H,W,seeds] values are in memory at once, so this is for short seed lists
    or small grids."""
    seeds = seeds_of(occ, of_clear)
    D, H, W = seeds.shape
    s = np.argwhere(seeds).astype(np.int64)
    if len(s) == 0:
        return np.full(seeds.shape, NONE, dtype=np.int32)
    dd = (np.arange(D)[:, None] - s[None, :, 0]) ** 2
    hh = (np.arange(H)[:, None] - s[None, :, 1]) ** 2
    ww = (np.arange(W)[:, None] - s[None, :, 2]) ** 2
    out = np.empty(seeds.shape, dtype=np.int64)
    for d in range(D):
        out[d] = (hh[:, None, :] + ww[None, :, :] + dd[d][None, None, :]).min(axis=2)
    return out.astype(np.int32)


def _along_last(seeds):
    """int64 [..., W]: squared distance along the last axis to the nearest seed of the line, _INF on a line without one
    (two sweeps: the last seed at or before w, the first at or after)."""
    W = seeds.shape[-1]
    idx = np.arange(W, dtype=np.int64)
    before = np.maximum.accumulate(np.where(seeds, idx, -1), axis=-1)
    after = np.minimum.accumulate(np.where(seeds, idx, 2 * W)[..., ::-1], axis=-1)[..., ::-1]
    left = np.where(before >= 0, idx - before, _INF)
    right = np.where(after < 2 * W, after - idx, _INF)
    d = np.minimum(left, right)
    return np.where(d < _INF, d * d, _INF)


def _min_plus(g, axis):
    """out(i) = min_j g(j) + (i - j)^2 along `axis`, one candidate j at a time (so a 128^3 grid stays within memory)."""
    g = np.moveaxis(g, axis, 0)
    n = g.shape[0]
    i = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * (g.ndim - 1))
    out = np.full(g.shape, _INF, dtype=np.int64)
    for j in range(n):
        np.minimum(out, g[j][None] + (i - j) ** 2, out=out)
    return np.moveaxis(out, 0, axis)


def edt_separable(occ, of_clear=False):
    """The same field by three separable integer passes (W, H, D)."""
    seeds = seeds_of(occ, of_clear)
    g = _min_plus(_min_plus(_along_last(seeds), 1), 0)
    return np.where(g < _INF, g, NONE).astype(np.int32)


def shell(occ):
    """The set voxels with at least one of their six face neighbours clear or outside the grid."""
    occ = np.asarray(occ, dtype=bool)
    p = np.pad(occ, 1, constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return occ & ~inner


def thresholds_sq(taus):
    t = np.asarray(list(taus), dtype=np.float64)
    return np.minimum(np.floor(t * t), float(NONE - 1)).astype(np.int32)


def edt_stats(sq, occ, thr_sq):
    """int64 [3 + K]: (n, reached, sum_sq, within_k ...) of the set voxels of occ in the field sq."""
    v = np.asarray(sq, dtype=np.int64)[np.asarray(occ, dtype=bool)]
    r = v[v != NONE]
    return np.array([len(v), len(r), r.sum()] + [(r <= int(t)).sum() for t in thr_sq], dtype=np.int64)


def surface_stats(pred, gt, thr_sq, surface=True, edt=edt_separable):
    """int64 [2, 3 + K]: row 0 the prediction's voxels in the ground truth's field, row 1 the reverse."""
    p, g = np.asarray(pred, dtype=bool), np.asarray(gt, dtype=bool)
    if surface:
        p, g = shell(p), shell(g)
    return np.stack([edt_stats(edt(g), p, thr_sq), edt_stats(edt(p), g, thr_sq)])


def fscore(stats):
    """float64 [..., K, 3] (precision, recall, F) of stats [..., 2, 3 + K]."""
    s = np.asarray(stats)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = s[..., 3:].astype(np.float64) / s[..., 0:1].astype(np.float64)
        prec, rec = share[..., 0, :], share[..., 1, :]
        total = prec + rec
        f = np.where(total == 0, 0.0, 2.0 * prec * rec / total)
    return np.stack([prec, rec, f], axis=-1)


def signed_sq(occ, edt=edt_separable):
    """(negative [D,H,W] bool, squared magnitude [D,H,W] int32) of the signed distance field: at an empty voxel + the
    distance to the nearest occupied one, at an occupied voxel - the distance to the nearest empty one."""
    occ = np.asarray(occ, dtype=bool)
    return occ, np.where(occ, edt(occ, True), edt(occ, False)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# seeded grids
CONTENTS = ("empty", "full", "corners", "single", "rand5", "rand50", "last_plane")


def grid(shape, kind, seed=0):
    """A bool [D,H,W] grid: empty, full, a voxel at each corner, one voxel alone, random at 5 % and 50 %, or voxels only in
    the plane d = D - 1 (so whole rows and planes have no seed)."""
    D, H, W = shape
    g = np.zeros(shape, dtype=bool)
    rng = np.random.default_rng([seed, D, H, W, CONTENTS.index(kind)])
    if kind == "full":
        g[:] = True
    elif kind == "corners":
        for c in np.ndindex(2, 2, 2):
            g[c[0] * (D - 1), c[1] * (H - 1), c[2] * (W - 1)] = True
    elif kind == "single":
        g[D - 1, 0, W // 2] = True
    elif kind == "rand5":
        g = rng.random(shape) < 0.05
    elif kind == "rand50":
        g = rng.random(shape) < 0.5
    elif kind == "last_plane":
        g[D - 1] = rng.random((H, W)) < 0.1
        g[D - 1, H - 1, W - 1] = True
    return g


def sparse_grid(shape, n, seed):
    """n distinct random voxels."""
    rng = np.random.default_rng([seed, n])
    g = np.zeros(shape, dtype=bool)
    g.reshape(-1)[rng.permutation(g.size)[:n]] = True
    return g


def ball(shape, centre, radius):
    """The voxels within `radius` of `centre` (index units)."""
    d, h, w = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (d - centre[0]) ** 2 + (h - centre[1]) ** 2 + (w - centre[2]) ** 2 <= radius * radius


def clouds_of_split(M, V, N, seed):
    """(predictions [(points [V,N,3] float32, num_points | None)] * M, gt clouds [n,3] float64 * M): noisy samples of a
    sphere per model, one model with truncated views."""
    rng = np.random.default_rng(seed)
    preds, gts = [], []
    for m in range(M):
        r = 0.25 + 0.05 * m
        u = rng.normal(size=(V, N, 3))
        pts = (r * u / np.linalg.norm(u, axis=2, keepdims=True) + 0.02 * rng.normal(size=(V, N, 3))).astype(np.float32)
        u = rng.normal(size=(400 + m, 3))
        gts.append(r * u / np.linalg.norm(u, axis=1, keepdims=True))
        preds.append((pts, np.array([N - 50, 0] + [N] * (V - 2))[:V] if m == 1 else None))
    return preds, gts


GOLDEN_SHAPES = ((1, 1, 1), (1, 1, 2), (3, 5, 7), (5, 33, 31), (2, 1, 40), (9, 16, 40))
GOLDEN_TAUS = (0.0, 1.0, 1.5, 2.0, 3.0)


def golden_cases():
    """(key, shape, kind, grid) of every recorded case."""
    for shape in GOLDEN_SHAPES:
        for kind in CONTENTS:
            yield "s%dx%dx%d_%s" % (shape + (kind,)), shape, kind, grid(shape, kind, 34)


def golden_partner(shape):
    """The grid every golden case of `shape` is compared with by the stats and the F-score."""
    return grid(shape, "rand5", 35)
