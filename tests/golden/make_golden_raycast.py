#!/usr/bin/env python3
"""Writes tests/golden/f33_raycast.npz: small meshes, ray bundles and the outputs of tests/raycast_oracle.py.  Runs on
the CPU in well under a minute:

    python tests/golden/make_golden_raycast.py

Per case <name>: <name>_O, <name>_D [n,3] (fp32 or fp64 as the name's suffix says), <name>_V [v,3] of the same dtype,
<name>_F [f,3] int32, <name>_range (t_min, t_max), and ray_mesh's <name>_t, _face, _weights, _hits, _normal.
generic: the names of the cases whose rays were drawn by rejection so that EVERY stored ray meets
raycast_oracle.clearance, conditions evaluated in exact arithmetic; on all of them the fp64 oracle's face and hits equal
the exact ones, asserted here.  dyadic: the names of the cases that are compared with the fp64 oracle bit for bit only.

    soup64, soup32   100 faces over 40 random vertices, three of them with repeated indices (zero area), 32 rays
    cube64, cube32   the unit cube wound outward, rays from inside and from outside
    open64, open32   the cube without its lid, t in [0.25, 1.75]
    dups64, dups32   the soup's first 30 faces with faces 1, 3 and 11 listed again at the end, 16 rays, six of them
                     sent at those faces from nearby so that they are first hits
    fan64, fan32     a planar fan of small dyadic coordinates; rays exactly through its shared vertex, its shared edges, its
                     outer vertices and edges, with hits exactly at t_min = 1 and t_max = 2 and just outside them: every
                     product is exact, so here too the oracle's face and hits equal the exact ones
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "pytorch-unsup-pc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import raycast_oracle as RO       # noqa: E402

DUP = (1, 3, 11)


def clear_rays(rng, n, V, F, t_range, dtype, aim=()):
    """n rays towards the mesh's box that meet the clearance conditions as values of dtype; ray k < len(aim) starts just
    off the point aim[k][0] along the unit vector aim[k][1], goes through that point's neighbourhood and has the face
    aim[k][2] for its first hit."""
    lo, hi = V.min(axis=0).astype(np.float64), V.max(axis=0).astype(np.float64)
    c, e = 0.5 * (lo + hi), float((hi - lo).max())
    O, D = [], []
    while len(O) < n:
        want = None
        if len(O) < len(aim):                               # from just off the face, and kept only when it is the first hit
            to, normal, want = aim[len(O)]
            to = to + rng.uniform(-0.02, 0.02, size=3) * e
            o = (to + (rng.choice([-0.03, 0.03]) * normal + rng.uniform(-0.005, 0.005, size=3)) * e).astype(dtype)
        else:
            to, o = rng.uniform(lo, hi), (c + rng.uniform(-1.2, 1.2, size=3) * e).astype(dtype)
        d = ((to - o) * rng.uniform(0.5, 2.0)).astype(dtype)
        if want is not None and RO.ray_mesh(o, d, V, F, *t_range)["face"][0] != want:
            continue
        if RO.clearance(o[None], d[None], V, F, *t_range)[0]:
            O.append(o)
            D.append(d)
    return np.asarray(O), np.asarray(D)


def fan_rays():
    xy = [(0, 0), (0.25, 0), (0.25, 0.25), (0, 0.25), (0.5, 0), (0.5, 0.5), (0.5, 0.25), (0.25, 0.125), (-0.125, -0.375), (0.75, 0),
          (-0.5, -0.5), (0.125, 0.125)]
    O, D = [], []
    for x, y in xy:
        for dz in (-1.0, -0.5, -2.0, -0.25, 1.0):        # t = 1, 2 (the bounds), 1/2 and 4 (outside them), -1 (behind)
            O.append((x, y, 1.0))
            D.append((0.0, 0.0, dz))
    for o, d in (((0.25, 0.125, 1.0), (0.25, 0.25, -1.0)), ((-0.5, 0.0, 1.5), (0.5, 0.0, -1.0)), ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
                 ((1.0, 0.25, 0.0), (-1.0, 0.0, 0.0)), ((0.0, 0.0, 2.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 2.0), (0.125, 0.0, -1.0))):
        O.append(o)
        D.append(d)
    return np.asarray(O, dtype=np.float64), np.asarray(D, dtype=np.float64)


def main():
    rng = np.random.default_rng(20240933)
    out, generic, dyadic = {}, [], []

    def add(name, O, D, V, F, t_range, kind):
        F = np.asarray(F, dtype=np.int32)
        res = RO.ray_mesh(O, D, V, F, *t_range)
        assert res["status"] == 0, name
        exact = RO.ray_mesh_exact(O, D, V, F, *t_range)
        assert [e["face"] for e in exact] == res["face"].tolist() and [e["hits"] for e in exact] == res["hits"].tolist(), name
        if kind is generic:
            assert RO.clearance(O, D, V, F, *t_range).all(), name
        out[name + "_O"], out[name + "_D"], out[name + "_V"], out[name + "_F"] = O, D, V, F
        out[name + "_range"] = np.asarray(t_range, dtype=np.float64)
        for k in ("t", "face", "weights", "hits", "normal"):
            out["%s_%s" % (name, k)] = res[k]
        kind.append(name)
        print("%-7s %3d rays %3d faces  hit %2d  hits histogram %s" % (name, len(O), len(F), int((res["face"] >= 0).sum()),
                                                                      np.bincount(res["hits"]).tolist()))

    V = rng.uniform(-0.5, 0.5, size=(40, 3))
    F = rng.integers(0, 40, size=(100, 3))
    F[10], F[50], F[90] = (3, 3, 7), (5, 5, 5), (8, 2, 8)
    Fd = np.concatenate([F[:30], F[list(DUP)]])
    cube_v, cube_f = RO.cube()
    _, open_f = RO.cube(lid=False)
    for suffix, dtype in (("64", np.float64), ("32", np.float32)):
        Vs, Vc = V.astype(dtype), cube_v.astype(dtype)
        add("soup" + suffix, *clear_rays(rng, 32, Vs, F, (0.0, np.inf), dtype), Vs, F, (0.0, np.inf), generic)
        add("cube" + suffix, *clear_rays(rng, 24, Vc, cube_f, (0.0, np.inf), dtype), Vc, cube_f, (0.0, np.inf), generic)
        add("open" + suffix, *clear_rays(rng, 24, Vc, open_f, (0.25, 1.75), dtype), Vc, open_f, (0.25, 1.75), generic)
        aim = [(V[F[j]].mean(axis=0), RO.C.face_normals(V, F[[j]])[0], j) for j in DUP + DUP]
        add("dups" + suffix, *clear_rays(rng, 16, Vs, Fd, (0.0, np.inf), dtype, aim), Vs, Fd, (0.0, np.inf), generic)
        assert set(out["dups%s_face" % suffix].tolist()) >= set(DUP), "the duplicated faces are first hits"
        fan_v, fan_f = RO.fan()
        O, D = fan_rays()
        assert (O.astype(np.float32) == O).all() and (D.astype(np.float32) == D).all() and (fan_v.astype(np.float32) == fan_v).all()
        add("fan" + suffix, O.astype(dtype), D.astype(dtype), fan_v.astype(dtype), fan_f, (1.0, 2.0), dyadic)
    assert (out["dups64_face"] < 30).all() and (out["dups32_face"] < 30).all(), "a duplicate listed later never wins"
    out["generic"], out["dyadic"] = np.array(generic), np.array(dyadic)
    path = os.path.join(HERE, "f33_raycast.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
