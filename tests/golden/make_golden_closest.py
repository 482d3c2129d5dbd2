#!/usr/bin/env python3
"""Writes tests/golden/f31_closest.npz: for the point-to-mesh cases of f28_point_mesh.npz (whose geometry it reuses and does
not store again) and two cases of its own, the exact closest point of every point (rational arithmetic, rounded once to
fp64), the exact least squared distance, the faces that attain it, and per case the worst error of the numpy oracle
(tests/closest_oracle.py) against them.  Runs on the CPU in about a minute:

    python tests/golden/make_golden_closest.py

Per case <name>: <name>_q [n,3] and <name>_d2 [n] (NaN / +inf: no usable face), <name>_argmin [n,K] int32 (the faces whose
exact d2 is the least, ascending, padded with -1) and <name>_near [n,K'] (those within a relative 1e-9 of it);
<name>_ratio_q, the worst error of the oracle's q against the stored <name>_q (the exact Q rounded once to fp64, which is
what a test compares with) in units of 2^-52 S (closest_oracle.unit_len), and <name>_ratio_wv, the same for sum w V rebuilt
in exact arithmetic from the oracle's weights.  The cases of its own also store
<name>_P, _V, _F:

    duplicates  one triangle listed with the same index triple at face j, j + face_tile (another tile) and
                j + chunk + 5 (another chunk of the split path); its points are nearest to it: the lowest index must win
    unique      points at a small height over face centroids of f28's icosphere; asserted here: the exact second-smallest
                d2 exceeds the smallest by more than a relative 1e-6 for every point, so the argmin is not in doubt

Asserted for every point of every case: all faces of <name>_near have the same exact closest point, so Q is unique and a
test can compare points whichever of those faces an implementation names.  Besides: cases (the names), well_shaped (all
but sliver), max_ratio_q / max_ratio_wv over the well-shaped cases, sliver's own ratios, and block, face_tile,
chunk_tiles: the library's constants the cases were placed from.

CAP.  The GPU tests allow 8 times a recorded ratio, so a case on which the oracle itself is poor would hand the kernel a
loose bound.  The oracle's q is a handful of fp64 operations on coordinates of magnitude <= S, each off by at most half a
unit, so a few units is what a sound case gives; CAP = 16 units -- make_golden_point_mesh.py's cap for the distance --
is where this script stops and the case is changed instead (the worst recorded here is below 1)."""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "pytorch-unsup-pc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import closest_oracle as C        # noqa: E402
import mesh_voxels_oracle as MV   # noqa: E402
import point_mesh_oracle as O     # noqa: E402
from dpc.render import _native    # noqa: E402

BLOCK, TILE, CHUNK = _native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE, _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
CAP = 16.0
REUSED = ("regions", "regions_p32", "cross", "tile_m1", "tile", "tile_p1", "tile_2p1", "blocks", "split", "mm", "degenerate_only",
          "degenerate_nearest", "sliver", "ico", "nan_among", "nan_only")
DUP_J = 3


def own_cases(f28):
    out = {}
    p0 = np.array([0.1, 0.2, -0.3])
    n = DUP_J + CHUNK + 5 + 20
    V, F = MV.soup(n, 31)
    V, F = V.copy(), F.copy()
    V[3 * DUP_J:3 * DUP_J + 3] = O.placed_face(p0).astype(np.float32)
    F[DUP_J + TILE] = F[DUP_J]
    F[DUP_J + CHUNK + 5] = F[DUP_J]
    P = np.stack([p0, p0 + (0.0005, 0.002, 0.001), p0 + (-0.001, 0.004, 0.003), p0 + (0.002, -0.012, 0.0)])
    out["duplicates"] = (P, V, F)
    iV, iF = f28["ico_V"], f28["ico_F"]
    c = iV[iF[:40]].mean(axis=1)
    out["unique"] = (c * (1.0 + 0.004 / np.linalg.norm(c, axis=1, keepdims=True)), iV, iF)
    return out


def padded(lists):
    k = max(1, max(len(x) for x in lists))
    return np.array([list(x) + [-1] * (k - len(x)) for x in lists], dtype=np.int32)


def main():
    f28 = dict(np.load(os.path.join(HERE, "f28_point_mesh.npz")))
    assert (int(f28["block"]), int(f28["face_tile"]), int(f28["chunk_tiles"])) == (BLOCK, TILE, _native.DPC_PM_CHUNK_TILES)
    out = {"block": BLOCK, "face_tile": TILE, "chunk_tiles": _native.DPC_PM_CHUNK_TILES, "dup_j": DUP_J}
    cases = {name: (f28[name + "_P"], f28[name + "_V"], f28[name + "_F"]) for name in REUSED}
    own = own_cases(f28)
    cases.update(own)
    worst_q = worst_wv = 0.0
    for name, (P, V, F) in cases.items():
        exact = C.mesh_closest_exact(P, V, F)
        d2, face, q, w, _ = C.mesh_closest(P, V, F)
        unit = C.unit_len(P, V)
        v64 = np.asarray(V).astype(np.float64)
        ratio_q = ratio_wv = 0.0
        for i, e in enumerate(exact):
            assert e["same_q"], (name, i, e["near"])
            if e["d2"] is None:
                assert face[i] == -1 and np.isinf(d2[i]) and np.isnan(q[i]).all() and np.isnan(w[i]).all(), (name, i)
                continue
            assert int(face[i]) in e["near"], (name, i, int(face[i]), e["near"])
            assert (w[i] >= 0).all(), (name, i, w[i])
            stored = [Fraction(float(x)) for x in e["q"]]                        # what <name>_q holds: the exact Q rounded once
            ratio_q = max(ratio_q, C.point_error(q[i], stored) / unit)
            ratio_wv = max(ratio_wv, C.point_error(C.combine_exact(w[i], v64[F[face[i]]]), stored) / unit)
        print("%-20s points %4d faces %5d ratio_q %.3f ratio_wv %.3f" % (name, len(P), len(F), ratio_q, ratio_wv), flush=True)
        assert ratio_q <= CAP, (name, ratio_q)
        if name != "sliver":
            assert ratio_wv <= CAP, (name, ratio_wv)
            worst_q, worst_wv = max(worst_q, ratio_q), max(worst_wv, ratio_wv)
        nan3 = [np.nan] * 3
        out.update({name + "_q": np.array([nan3 if e["q"] is None else [float(x) for x in e["q"]] for e in exact]),
                    name + "_d2": O.rounded([e["d2"] for e in exact]), name + "_argmin": padded([e["argmin"] for e in exact]),
                    name + "_near": padded([e["near"] for e in exact]), name + "_ratio_q": ratio_q, name + "_ratio_wv": ratio_wv})
        if name in REUSED:
            assert np.array_equal(out[name + "_d2"], f28[name + "_d2"]), name                # the same exact distances
        else:
            out.update({name + "_P": P, name + "_V": V, name + "_F": np.asarray(F, dtype=np.int32)})
        if name == "duplicates":
            want = [DUP_J, DUP_J + TILE, DUP_J + CHUNK + 5]
            assert all(e["argmin"] == want and e["near"] == want for e in exact), [e["argmin"] for e in exact]
            assert (face == DUP_J).all()
        if name == "unique":
            for i, e in enumerate(exact):
                assert e["argmin"] == [i] and e["near"] == [i], (i, e["argmin"])
                assert e["second"] is None or e["second"] > e["d2"] * (1 + 1e-6), (i, float(e["second"]), float(e["d2"]))
    out.update({"cases": np.array(list(cases)), "well_shaped": np.array([n for n in cases if n != "sliver"]),
                "max_ratio_q": worst_q, "max_ratio_wv": worst_wv})
    print("max ratio_q %.3f max ratio_wv %.3f (well-shaped); sliver ratio_q %.3f ratio_wv %.3f"
          % (worst_q, worst_wv, out["sliver_ratio_q"], out["sliver_ratio_wv"]))
    path = os.path.join(HERE, "f31_closest.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes; f28_point_mesh.npz has %d)" % (path, os.path.getsize(path), os.path.getsize(os.path.join(HERE, "f28_point_mesh.npz"))))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "f28_point_mesh.npz"))


if __name__ == "__main__":
    main()
