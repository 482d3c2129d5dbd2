"""Numpy restatement of the voxel-grid conventions of include/dpc_render.h (dpc_voxelise): the voxelisation rule, the bit
layout, the thresholds, the five counts and voxel2pc, plus the seeded inputs the voxel tests and the fixture
tests/golden/f25_voxels.npz share.  Everything here is exact: integers, bits, and elementwise fp64 arithmetic."""
import hashlib

import numpy as np

STAT_NAMES = ("diff", "intersection", "union", "num_fp", "num_fn")


def shape_of(vox_size, vox_size_z=-1):
    return (vox_size if vox_size_z == -1 else vox_size_z, vox_size, vox_size)


def nodes(points, shape):
    """(valid [n] bool, idx [n,3] int64: the node of every valid point, 0 elsewhere)."""
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        valid = ((p >= -0.5) & (p <= 0.5)).all(axis=1)
    idx = np.zeros(p.shape, dtype=np.int64)
    G1 = np.asarray(shape, dtype=np.float64) - 1.0
    t = (p[valid] + 0.5) * G1
    idx[valid] = np.floor(t + 0.5).astype(np.int64)
    return valid, idx


def voxelise(points, shape):
    """(bool [D,H,W] grid, dropped points) of one cloud."""
    valid, idx = nodes(points, shape)
    grid = np.zeros(shape, dtype=bool)
    i = idx[valid]
    grid[i[:, 0], i[:, 1], i[:, 2]] = True
    return grid, int((~valid).sum())


def pack_bits(mask):
    """uint32 words of a bool grid: voxel f (C order) is bit f & 31 of word f >> 5, padding bits zero."""
    flat = np.asarray(mask, dtype=bool).reshape(-1)
    words = (len(flat) + 31) // 32
    padded = np.zeros(words * 32, dtype=np.uint8)
    padded[:len(flat)] = flat
    return np.packbits(padded.reshape(words, 32), axis=1, bitorder="little").view("<u4").reshape(words)


def threshold(grid, thr, inclusive):
    """occupied = grid >= thr (inclusive) or grid > thr, in the grid's own dtype with thr rounded to it; NaN unoccupied."""
    g = np.asarray(grid)
    t = g.dtype.type(thr)
    with np.errstate(invalid="ignore"):
        return (g >= t) if inclusive else (g > t)


def stats(p, g):
    """The five counts of a pair of bool grids, int64."""
    p, g = np.asarray(p, dtype=bool), np.asarray(g, dtype=bool)
    return np.array([(p ^ g).sum(), (p & g).sum(), (p | g).sum(), (p & ~g).sum(), (~p & g).sum()], dtype=np.int64)


def iou(s):
    s = np.asarray(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s[..., 2] > 0, s[..., 1].astype(np.float64) / s[..., 2].astype(np.float64), np.nan)


def evaluate_voxel_prediction(preds, gt, thresh):
    """[B,2,D,H,W] arrays: the counts of (preds[:,1] >= thresh) against gt's channel 1 as logical, num_fp against channel 0."""
    occ = threshold(preds[:, 1], thresh, True)
    g1, g0 = gt[:, 1] != 0, gt[:, 0] != 0
    s = stats(occ, g1)
    return np.array([s[0], s[1], s[2], (occ & g0).sum(), s[4]], dtype=np.int64)


def axis_coordinates(G):
    x = np.arange(G, dtype=np.float64) * (1.0 / (G - 1)) + (-0.5)
    x[G - 1] = 0.5
    return x


def voxel2pc(voxels, thr):
    """(xyz [n,3] float64, occupancies [G^3] bool): voxel (i,j,k) at (x[j], x[i], x[k]), ascending flat index."""
    v = np.squeeze(np.asarray(voxels))
    G = v.shape[0]
    if v.ndim != 3 or v.shape != (G, G, G) or G < 2:
        raise ValueError("voxel2pc needs a cubic grid with G >= 2, got %s" % (v.shape,))
    if v.dtype not in (np.float32, np.float64):
        v = v.astype(np.float64)
    occ = threshold(v, thr, False).reshape(-1)
    i, j, k = np.unravel_index(np.flatnonzero(occ), (G, G, G))
    x = axis_coordinates(G)
    return np.stack([x[j], x[i], x[k]], axis=1).reshape(-1, 3), occ


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs
def cloud(n, seed, dtype=np.float32, shape=None):
    """n points: most inside the unit cube, some exactly on its faces, just outside it, and (given a grid shape) exactly
    half-way between two nodes of every axis."""
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) * 1.1 - 0.55).astype(dtype)
    special = [(0.5, 0.5, 0.5), (-0.5, -0.5, -0.5), (0.5, -0.5, 0.25), (np.nextafter(dtype(0.5), dtype(1)), 0.0, 0.0),
               (0.0, np.nextafter(dtype(-0.5), dtype(-1)), 0.0), (np.nextafter(dtype(0.5), dtype(0)), 0.1, -0.1)]
    if shape is not None:
        for c in range(3):
            if shape[c] > 1 and ((shape[c] - 1) & (shape[c] - 2)) == 0:   # G - 1 a power of two: (m + 0.5) / (G - 1) is exact
                q = [0.125, -0.25, 0.375]
                q[c] = (1 + 0.5) / (shape[c] - 1) - 0.5 if shape[c] > 2 else 0.0
                special.append(tuple(q))
    for r, s in zip(rng.permutation(n)[:len(special)], special):
        p[r] = s
    return p


def float_grids(B, shape, seed, dtype, thresholds=(0.3, 0.5), occupancy=None):
    """[B,D,H,W] values in [0, 1) with voxels set exactly to every threshold rounded to dtype, one step above and below
    it, and a NaN.  occupancy: about that share of the voxels is above 0.5, the rest below 0.25."""
    rng = np.random.default_rng(seed)
    g = rng.random((B,) + tuple(shape))
    if occupancy is not None:
        g = np.where(rng.random(g.shape) < occupancy, 0.5 + 0.5 * g, 0.25 * g)
    g = g.astype(dtype)
    flat = g.reshape(B, -1)
    values = [v for t in thresholds for v in (dtype(t), np.nextafter(dtype(t), dtype(1)), np.nextafter(dtype(t), dtype(0)))] + [dtype("nan")]
    if flat.shape[1] >= 2 * len(values):
        for b in range(B):
            where = rng.permutation(flat.shape[1])[:len(values)]
            flat[b, where] = values
    return flat.reshape(g.shape)


def prediction_pair(B, G, seed, dtype):
    """(preds, gt) [B,2,G,G,G] as evaluate_voxel_prediction takes them: gt's channel 1 a 0 / 1 occupancy, channel 0 its
    complement, with a few voxels set in both or in neither."""
    rng = np.random.default_rng(seed)
    preds = np.stack([float_grids(B, (G, G, G), seed + 1, dtype), float_grids(B, (G, G, G), seed + 2, dtype)], axis=1)
    occ = rng.random((B, G, G, G)) < 0.4
    gt = np.stack([~occ, occ], axis=1).astype(dtype)
    flat = gt.reshape(B, 2, -1)
    flat[:, 0, 0] = 1
    flat[:, 1, 0] = 1
    flat[:, 0, -1] = 0
    flat[:, 1, -1] = 0
    return preds, gt


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


GOLDEN_SIDES = (2, 3, 5, 33)
GOLDEN_THRESHOLDS = (0.3, 0.5)
GOLDEN_DTYPES = ("float32", "float64")


def golden_cases():
    """(key, G, threshold, dtype, seed) of every recorded case."""
    for G in GOLDEN_SIDES:
        for t in GOLDEN_THRESHOLDS:
            for name in GOLDEN_DTYPES:
                yield "g%d_t%d_%s" % (G, round(t * 10), name), G, t, np.dtype(name).type, 1000 * G + round(t * 10) + (name == "float64")


def golden_inputs(G, seed, dtype):
    """(voxels [1,G,G,G,1] for voxel2pc, preds, gt [2,2,G,G,G] for evaluate_voxel_prediction)."""
    voxels = float_grids(1, (G, G, G), seed, dtype).reshape(1, G, G, G, 1)
    preds, gt = prediction_pair(2, G, seed + 7, dtype)
    return voxels, preds, gt
