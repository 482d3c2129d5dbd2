#!/usr/bin/env python3
"""Writes tests/golden/f32_winding.npz: small meshes, query points and the winding sums of tests/winding_oracle.py with
every term evaluated at 50 digits before it is quantised (mesh_sums_mp).  Runs on the CPU in about a minute:

    python tests/golden/make_golden_winding.py

Per case <name>: <name>_P [n,3], <name>_V [v,3], <name>_F [f,3] int32, <name>_sums [n] int64 (the mpmath sums),
<name>_bound (the most a device sum may differ from them, in quanta: the usable faces, winding_oracle.bound) and
<name>_clearance (the least distance of a point to the surface over the mesh's extent, the longest side of its bounding
box).  cases: the names; clear: those whose points keep CLEARANCE = 1e-3 of the extent from the surface, asserted here with
point_mesh_oracle -- the bound holds for these; exact: the guard cases whose points lie on the surface on purpose.

    soup64, soup32   97 faces over 40 random vertices, four of them with repeated indices (zero area), 60 points; fp64
                     coordinates, and the same rounded to fp32 (stored as fp32)
    cube, cube_in    a generically placed box wound outward (w = 1 inside, 0 outside) and inward (-1, 0)
    tetra, tetra_in  a tetrahedron likewise
    on_vertex        the cube, and points exactly on its vertices: the three faces at the vertex contribute 0
    in_plane         the cube, and points exactly in the planes of its sides, inside a side, beside it, and on an edge

Asserted: numpy's sums (mesh_sums) are within the bound of the mpmath sums on every clear case (they are equal on all of
them here), and the closed meshes give exactly 2^40, -2^40 or 0 within the bound."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "pytorch-unsup-pc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import point_mesh_oracle as O     # noqa: E402
import winding_oracle as WO       # noqa: E402

ONE = 1 << WO.FRAC_BITS
LO, HI = WO.VOX_LO, WO.VOX_HI


def extent(V):
    v = np.asarray(V).astype(np.float64)
    return float((v.max(axis=0) - v.min(axis=0)).max())


def clearance(P, V, F):
    d2, _ = O.mesh_d2(P, V, F)
    return float(np.sqrt(d2.min()) / extent(V))


def clear_points(rng, n, V, F, lo, hi):
    """n points uniform in [lo, hi]^3 that keep twice the clearance from the surface (the fp32 copy moves them a little)."""
    out = []
    while len(out) < n:
        p = rng.uniform(lo, hi, size=(1, 3))
        if clearance(p, V, F) >= 2.0 * WO.CLEARANCE:
            out.append(p[0])
    return np.asarray(out)


def main():
    rng = np.random.default_rng(20240607)
    out, cases, clear, exact = {}, [], [], []

    def add(name, P, V, F, is_clear):
        sums, status = WO.mesh_sums_mp(P, V, F)
        assert status == 0, name
        out[name + "_P"], out[name + "_V"], out[name + "_F"] = P, V, np.asarray(F, dtype=np.int32)
        out[name + "_sums"] = sums
        out[name + "_bound"] = np.int64(WO.bound(V, F))
        out[name + "_clearance"] = np.float64(clearance(P, V, F))
        cases.append(name)
        (clear if is_clear else exact).append(name)
        numpy_sums, _ = WO.mesh_sums(P, V, F)
        worst = int(np.abs(numpy_sums - sums).max())
        if is_clear:
            assert out[name + "_clearance"] >= WO.CLEARANCE, (name, out[name + "_clearance"])
            assert worst <= WO.bound(V, F), (name, worst)
        else:
            assert worst == 0, (name, worst)
        print("%-10s %3d points %3d faces  clearance %.2e  numpy - mpmath: %d quanta" % (name, len(P), len(F), out[name + "_clearance"], worst))
        return sums

    V = rng.uniform(-0.5, 0.5, size=(40, 3))
    F = rng.integers(0, 40, size=(97, 3))
    F[10], F[50], F[90], F[96] = (3, 3, 7), (5, 5, 5), (8, 2, 8), (1, 9, 9)
    P = clear_points(rng, 60, V, F, -0.6, 0.6)
    add("soup64", P, V, F, True)
    add("soup32", P.astype(np.float32), V.astype(np.float32), F, True)

    for name, (Vc, Fc) in (("cube", WO.cube(LO, HI)), ("tetra", WO.tetrahedron())):
        c, e = Vc.mean(axis=0), extent(Vc)
        P = clear_points(rng, 40, Vc, Fc, float(Vc.min()) - 0.2 * e, float(Vc.max()) + 0.2 * e)
        P[0] = c
        for k in range(1, 10):                              # both meshes are convex: points half-way to a random inner point
            P[k] = c + 0.5 * (rng.dirichlet(np.ones(len(Vc))) @ Vc - c)
        assert clearance(P, Vc, Fc) >= WO.CLEARANCE
        s_out = add(name, P, Vc, Fc, True)
        s_in = add(name + "_in", P, Vc, Fc[:, ::-1].copy(), True)
        n = len(Fc)
        assert s_out[0] != 0 and (np.minimum(np.abs(s_out - ONE), np.abs(s_out)) <= n).all(), name
        assert (np.minimum(np.abs(s_in + ONE), np.abs(s_in)) <= n).all() and (np.abs(s_in + s_out) <= n).all(), name
        assert 5 <= int((np.abs(s_out - ONE) <= n).sum()) <= 35, name                       # points on both sides

    Vc, Fc = WO.cube(LO, HI)
    add("on_vertex", Vc[[0, 3, 5, 6]].copy(), Vc, Fc, False)
    mid = 0.5 * (np.asarray(LO) + np.asarray(HI))
    P = np.array([[LO[0], mid[1], mid[2]], [HI[0], mid[1] + 0.01, mid[2]], [mid[0], LO[1], mid[2] - 0.02], [mid[0], mid[1], HI[2]],
                  [LO[0], HI[1] + 0.25, mid[2]], [mid[0], LO[1], HI[2] + 0.125], [LO[0], LO[1], mid[2]]])
    add("in_plane", P, Vc, Fc, False)

    out["cases"], out["clear"], out["exact"] = np.array(cases), np.array(clear), np.array(exact)
    out["clearance"] = np.float64(WO.CLEARANCE)
    out["frac_bits"] = np.int64(WO.FRAC_BITS)
    path = os.path.join(HERE, "f32_winding.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
