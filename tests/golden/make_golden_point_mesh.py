#!/usr/bin/env python3
"""Writes tests/golden/f28_point_mesh.npz: the inputs of the point-to-mesh cases, their exact squared distances (rational
arithmetic, rounded once to fp64), and per case the worst error of the numpy oracle against them in units of 2^-52 S^2
(tests/point_mesh_oracle.py: unit()).  The GPU test allows 8 times the largest recorded ratio; this script asserts that
it is at most 16 -- when a case breaks that, the case changes, not the cap.  Runs on the CPU in about a minute:

    python tests/golden/make_golden_point_mesh.py

Per case <name>: <name>_P [n,3], <name>_V [v,3], <name>_F [f,3] int32, <name>_d2 [n] fp64 (+inf: no face left),
<name>_ratio (a scalar).  random_T [60,3,3] / random_P [60,4,3] / random_d2 [60,4] / random_ratio: sixty one-triangle rows of
random triangles and points in the cube, the sample the tolerance mostly rests on.  Besides: max_ratio; block, face_tile,
chunk_tiles (the library's constants the boundary cases were placed from); ico_radii; the F-score case fs_* with
fs_thresholds and fs_margin (no exact squared distance is nearer to a squared threshold than fs_margin units,
asserted here)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "pytorch-unsup-pc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import mesh_voxels_oracle as MV   # noqa: E402
import point_mesh_oracle as O     # noqa: E402
from dpc.render import _native    # noqa: E402

BLOCK, TILE, CHUNK = _native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE, _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
CAP = 16.0
FS_MARGIN = 1.0e4

TRI = np.array([[-0.3, -0.2, -0.1], [0.25, 0.1, -0.2], [0.0, 0.3, 0.35]])
F1 = np.array([[0, 1, 2]], dtype=np.int32)


def region_points(tri, lift):
    """A point over each of the seven regions of the triangle (interior, three edges, three vertices), lifted by +lift and
    -lift along the normal."""
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    n /= np.linalg.norm(n)
    bary = [(1 / 3, 1 / 3, 1 / 3), (0.5, 0.7, -0.2), (-0.25, 0.6, 0.65), (0.55, -0.3, 0.75), (1.6, -0.3, -0.3), (-0.2, 1.5, -0.3),
            (-0.4, -0.3, 1.7)]
    base = np.array([b[0] * tri[0] + b[1] * tri[1] + b[2] * tri[2] for b in bary])
    return np.concatenate([base + lift * n, base - lift * n])


def soup_with(n, seed, placed):
    """A soup of n faces (fp32) in which face index i is replaced by the triangle placed[i] ([3,3])."""
    V, F = MV.soup(n, seed)
    V = V.copy()
    for i, tri in placed.items():
        V[3 * i:3 * i + 3] = tri.astype(np.float32)
    return V, F


def cases():
    rng = np.random.default_rng(28)
    out = {}
    out["regions"] = (region_points(TRI, 0.15), TRI, F1)
    out["regions_p32"] = (region_points(TRI, 0.15).astype(np.float32), TRI, F1)
    flat = np.array([[-0.25, -0.25, 0.125], [0.25, -0.25, 0.125], [-0.25, 0.25, 0.125]])
    on = np.array([[-0.125, -0.125, 0.125], [0.0, -0.25, 0.125], [0.0, 0.0, 0.125], [-0.25, -0.25, 0.125], [0.25, -0.25, 0.125],
                   [-0.25, 0.25, 0.125], [-0.125, -0.125, 0.375], [0.375, -0.375, 0.125]])
    out["on_triangle"] = (on, flat, F1)
    # zero-area faces only: collinear, a point, two vertices coincident (both ways round)
    dV = np.array([[-0.4, -0.4, -0.4], [0.4, 0.4, 0.4], [0.0, 0.0, 0.0], [0.2, -0.3, 0.1], [0.2, -0.3, 0.4]])
    dF = np.array([[0, 1, 2], [3, 3, 3], [3, 4, 4], [3, 4, 3], [2, 0, 1]], dtype=np.int32)
    dP = np.concatenate([rng.random((12, 3)) - 0.5, [[0.2, -0.3, 0.25], [0.1, 0.1, 0.1], [0.5, 0.5, 0.5], [0.2, -0.3, 0.1]]])
    out["degenerate_only"] = (dP, dV, dF)
    # a zero-area face (a segment) that is the nearest face of its mesh
    sV, sF = MV.soup(20, 3)
    seg = np.array([[0.11, 0.21, -0.31], [0.13, 0.24, -0.27], [0.13, 0.24, -0.27]], dtype=np.float32)
    gV, gF = MV.join((sV, sF), (seg, F1))
    out["degenerate_nearest"] = (np.array([[0.12, 0.22, -0.29], [0.10, 0.20, -0.33], [0.2, 0.3, -0.2]]), gV, gF)
    # face-tile boundaries: the nearest face of point 0 is the last one
    p0 = np.array([0.1, 0.2, -0.3])
    for name, n in (("tile_m1", TILE - 1), ("tile", TILE), ("tile_p1", TILE + 1), ("tile_2p1", 2 * TILE + 1)):
        V, F = soup_with(n, 40 + n, {n - 1: O.placed_face(p0)})
        out[name] = (np.stack([p0, rng.random(3) - 0.5]), V, F)
    out["cross"] = (out["tile_p1"][0], TRI, F1)
    # point-block boundaries: BLOCK + 1 fp32 points on an fp32 mesh; the test issues the first 1, BLOCK - 1, BLOCK, BLOCK + 1
    iV, iF = MV.icosphere(0, 0.35, (0.02, -0.01, 0.03), np.float32)
    out["blocks"] = ((rng.random((BLOCK + 1, 3)) - 0.5).astype(np.float32), iV, iF)
    # the split path: 3 points, 4 chunks and one face; the nearest faces lie in the first, an inner and the last chunk
    sp = np.array([[0.1, 0.2, -0.3], [-0.2, 0.15, 0.25], [0.3, -0.35, 0.05]])
    n = 4 * CHUNK + 1
    V, F = soup_with(n, 7, {5: O.placed_face(sp[0]), 2 * CHUNK + 7: O.placed_face(sp[1]), n - 1: O.placed_face(sp[2])})
    out["split"] = (sp, V, F)
    # scale: a millimetre triangle with points a millimetre away, and a sliver 1e-6 wide
    c = np.array([0.31, -0.27, 0.18])
    mm = c + (rng.random((3, 3)) - 0.5) * 2e-3
    d = rng.normal(size=(40, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out["mm"] = (np.concatenate([mm.mean(axis=0) + 1e-3 * d[:30], mm.mean(axis=0) + 1e-4 * d[30:]]), mm, F1)
    a, b = np.array([-0.3, -0.2, 0.1]), np.array([0.4, 0.3, -0.2])
    perp = np.cross(b - a, [0.0, 0.0, 1.0])
    sl = np.stack([a, b, a + 0.37 * (b - a) + 1e-6 * perp / np.linalg.norm(perp)])
    out["sliver"] = (np.concatenate([rng.random((30, 3)) - 0.5, sl.mean(axis=0) + 1e-4 * d[:10]]), sl, F1)
    # an icosphere of radius R, points at radius r along vertex directions
    R_, r_ = 0.3, 0.45
    V, F = MV.icosphere(2, R_)
    out["ico"] = (V[:30] / np.linalg.norm(V[:30], axis=1, keepdims=True) * r_, V, F)
    # non-finite vertices: one such face among good ones, and a mesh of such faces only
    nV, nF = MV.soup(10, 11, dtype=np.float64)
    bad = np.array([[0.0, 0.0, 0.0], [np.nan, 0.1, 0.1], [0.1, 0.0, 0.1]])
    nP = rng.random((6, 3)) - 0.5
    out["nan_without"] = (nP, nV, nF)
    out["nan_among"] = (nP,) + MV.join((nV[:12], nF[:4]), (bad, F1), (nV[12:], nF[4:] - 12))
    out["nan_only"] = (nP[:3], np.array([[0.0, 0.0, 0.0], [np.inf, 0.1, 0.1], [0.1, 0.0, 0.1], [np.nan, 0.0, 0.0]]),
                       np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
    return out, (R_, r_)


def fscore_case():
    rng = np.random.default_rng(281)
    V, F = MV.icosphere(1, 0.3)
    gt = MV.face_points(V, F, 2, 5)[::3]
    d = rng.normal(size=(2, 60, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    preds = d * (0.29 + 0.03 * rng.random((2, 60, 1)))
    return preds, gt, V, F, np.array([0.004, 0.01, 0.02])


def main():
    out = {"block": BLOCK, "face_tile": TILE, "chunk_tiles": _native.DPC_PM_CHUNK_TILES}
    all_cases, (R_, r_) = cases()
    worst = 0.0
    for name, (P, V, F) in all_cases.items():
        exact = O.rounded(O.mesh_d2_exact(P, V, F))
        got, _ = O.mesh_d2(P, V, F)
        fin = np.isfinite(exact)
        assert (np.isfinite(got) == fin).all(), name
        ratio = float((np.abs(got[fin] - exact[fin]) / O.unit(P, V)).max()) if fin.any() else 0.0
        print("%-20s points %4d faces %5d ratio %.3f" % (name, len(P), len(F), ratio), flush=True)
        assert ratio <= CAP, (name, ratio)
        worst = max(worst, ratio)
        out.update({name + "_P": P, name + "_V": V, name + "_F": np.asarray(F, dtype=np.int32), name + "_d2": exact,
                    name + "_ratio": ratio})
    # what the cases were built for
    assert (out["on_triangle_d2"][:6] == 0.0).all() and out["on_triangle_d2"][6] == 0.0625
    for name in ("tile_m1", "tile", "tile_p1", "tile_2p1"):
        P, V, F = all_cases[name]
        assert O.tri_d2(P[:1], *(V[F[:, k]] for k in range(3)))[0].argmin() == len(F) - 1, name
    P, V, F = all_cases["split"]
    assert O.tri_d2(P, *(V[F[:, k]] for k in range(3))).argmin(axis=1).tolist() == [5, 2 * CHUNK + 7, len(F) - 1]
    P, V, F = all_cases["degenerate_nearest"]
    assert O.tri_d2(P[:2], *(V[F[:, k]] for k in range(3))).argmin(axis=1).tolist() == [len(F) - 1] * 2
    assert (out["nan_among_d2"] == out["nan_without_d2"]).all() and np.isinf(out["nan_only_d2"]).all()
    assert (np.sqrt(out["ico_d2"]) >= r_ - R_ - 1e-12).all()
    out["ico_radii"] = np.array([R_, r_])
    # random triangles in the unit cube, one row each (a batch of many small meshes): the sample the tolerance rests on
    rng = np.random.default_rng(2028)
    rT, rP = rng.random((60, 3, 3)) - 0.5, rng.random((60, 4, 3)) - 0.5
    rd2, ratio = np.zeros((60, 4)), 0.0
    for k in range(60):
        rd2[k] = O.rounded(O.mesh_d2_exact(rP[k], rT[k], F1))
        ratio = max(ratio, float((np.abs(O.mesh_d2(rP[k], rT[k], F1)[0] - rd2[k]) / O.unit(rP[k], rT[k])).max()))
    print("%-20s points %4d faces %5d ratio %.3f" % ("random", 240, 60, ratio), flush=True)
    assert ratio <= CAP, ratio
    worst = max(worst, ratio)
    out.update({"random_P": rP, "random_T": rT, "random_d2": rd2, "random_ratio": ratio})
    preds, gt, V, F, thr = fscore_case()
    for k in range(2):
        exact = O.rounded(O.mesh_d2_exact(preds[k], V, F))
        gap = np.abs(exact[:, None] - (thr ** 2)[None, :]).min() / O.unit(preds[k], V)
        assert gap > FS_MARGIN, gap
        out["fs_pred%d" % k] = preds[k]
        out["fs_pred%d_d2" % k] = exact
        got, _ = O.mesh_d2(preds[k], V, F)
        ratio = float((np.abs(got - exact) / O.unit(preds[k], V)).max())
        assert ratio <= CAP
        worst = max(worst, ratio)
    out.update({"fs_gt": gt, "fs_V": V, "fs_F": F, "fs_thresholds": thr, "fs_margin": FS_MARGIN, "max_ratio": worst})
    print("max ratio %.3f" % worst)
    path = os.path.join(HERE, "f28_point_mesh.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
