#!/usr/bin/env python3
"""Time of the ray-mesh intersection (dpc.render.raycast, csrc/dpc_raycast.hip) against the same rule composed from torch
ops on the same device, at two shapes:

    rays     ray_mesh_intersect of 100 000 fp32 rays against one mesh of 20 000 faces (bench_winding's points shape, so
             the two brute-force walks can be read side by side)
    visible  visible_points of 32 meshes of 1 280 faces with 8 000 fp32 surface samples each, one viewpoint per mesh

Per shape: the wall time of the Python call (packing and upload included), the library's launch record (k_rc_*,
k_pm_scan), the (ray, face) pairs per second of the wall time and of the kernels, and the composition's wall time --
torch_hits below, the rule of include/dpc_render.h (dpc_ray_mesh_intersect) in fp64 torch ops, at most --pairs (ray,
face) pairs at a time so that its [R,F,3] temporaries fit.  The composition's face and hits are compared with the
kernel's before anything is timed, and the number of rays that differ is recorded (torch may fuse or reorder nothing
either, so none is expected).  One JSON line per shape, appended to profiles/raycast_bench.jsonl (--out).

    python tools/bench_raycast.py [--reps 3] [--pairs 16777216]
    python tools/bench_raycast.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import bench_winding as BW
import numpy as np

RAYS_SHAPE = BW.POINTS_SHAPE          # rays, faces
VISIBLE_SHAPE = (32, 8000)            # meshes, samples per mesh
VISIBLE_FACES = BW.VOXEL_FACES
EPS = 1e-5                            # fp32 samples of meshes of size ~0.8, seen from a distance of ~2
mesh = BW.mesh


def resource_usage(path):
    BL.resource_usage("dpc_raycast.hip", path, [
        "# k_rc_hit<fp64 rays, fp64 vertices>: lds= is the face tile, DPC_PM_FACE_TILE records of 5 double2 (static);",
        "# k_rc_finish<fp64 rays, fp64 vertices>: one lane per output ray; k_pm_scan<1>: this file's copy of the shared scan"])


def torch_hits(O, D, tri, t_min, t_max, pairs):
    """(t [n] fp64, face [n] int64, hits [n] int64) of the rays O + t D [n,3] fp64 against the triangles tri [f,3,3] fp64 on
    the device, from torch ops, at most `pairs` (ray, face) pairs at a time."""
    import torch

    n = len(O)
    t_out = torch.empty((n,), dtype=torch.float64, device=O.device)
    face, hits = (torch.empty((n,), dtype=torch.int64, device=O.device) for _ in range(2))
    step = max(1, pairs // max(1, len(tri)))
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    cross = lambda x, y: torch.stack(torch.broadcast_tensors(x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                                                             x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]), dim=-1)
    v0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=O.device)
    for s in range(0, n, step):
        o, d = O[s:s + step, None, :], D[s:s + step, None, :]
        pv = cross(d, e2)
        det = dot(e1, pv)
        T = o - v0
        a = dot(T, pv)
        q = cross(T, e1)
        b = dot(d, q)
        sign = torch.where(det > 0, 1.0, -1.0)
        sa, sb, m = sign * a, sign * b, det.abs()
        inside = (m > 0) & (sa >= 0) & (sb >= 0) & (sa + sb <= m)
        t = dot(e2, q) / torch.where(inside, det, torch.ones_like(det))
        hit = inside & (t >= t_min) & (t <= t_max)
        th = torch.where(hit, t, inf)
        best = th.min(dim=1).values
        first = (th == best[:, None]).to(torch.int8).argmax(dim=1)      # the lowest index among equal t
        t_out[s:s + step] = best
        face[s:s + step] = torch.where(torch.isinf(best), torch.full_like(first, -1), first)
        hits[s:s + step] = hit.sum(dim=1)
    return t_out, face, hits


def kernels(fn, dev):
    return BL.kernel_ms(fn, dev, ("k_rc_", "k_pm_scan"))


def rates(out, pairs):
    out["pairs"] = int(pairs)
    out["kernel_ms_total"] = round(sum(out["kernel_ms"].values()), 4)
    out["gpairs_per_s_wall"] = round(pairs / out["wall_ms_median_min_max"][0] * 1e-6, 3)
    out["gpairs_per_s_kernel"] = round(pairs / out["kernel_ms_total"] * 1e-6, 3)
    out["torch_over_wall"] = round(out["torch_wall_ms_median_min_max"][0] / out["wall_ms_median_min_max"][0], 3)
    return out


def bench_rays(a, torch, dev):
    import dpc.render as R

    n, f = RAYS_SHAPE
    V, F = mesh(f)
    rng = np.random.default_rng(5)
    O = ((rng.random((n, 3)) - 0.5) * 2.0).astype(np.float32)
    D = ((rng.random((n, 3)) - 0.5) * 0.8 - O).astype(np.float32)      # towards the mesh, not normalised
    run = lambda: R.ray_mesh_intersect([O], [D], [(V, F)])
    Od, Dd = (torch.from_numpy(x).to(dev).double() for x in (O, D))
    tri = torch.from_numpy(V.astype(np.float64)[F]).to(dev)
    comp = lambda: torch_hits(Od, Dd, tri, 0.0, float("inf"), a.pairs)
    got, (t, face, hits) = run()[0], comp()
    out = {"bench": "raycast", "shape": "rays", "rays": n, "faces": f, "reps": a.reps, "torch_pairs_per_step": a.pairs,
           "rays_whose_face_differs_from_torch": int((got.face.long() != face).sum()),
           "rays_whose_hits_differ_from_torch": int((got.hits.long() != hits).sum()),
           "rays_whose_t_differs_from_torch": int((got.t != t).sum()), "rays_that_hit": int((got.face >= 0).sum()),
           "mean_hits": round(float(got.hits.double().mean()), 3),
           "wall_ms_median_min_max": BL.median_ms(run, a.reps), "kernel_ms": kernels(run, dev),
           "torch_wall_ms_median_min_max": BL.median_ms(comp, a.reps), "device": torch.cuda.get_device_name(0)}
    return rates(out, n * f)


def bench_visible(a, torch, dev):
    import dpc.render as R

    M, n = VISIBLE_SHAPE
    meshes = [mesh(VISIBLE_FACES, 100 + m) for m in range(M)]
    rng = np.random.default_rng(6)
    clouds, views = [], []
    for V, F in meshes:                                                # samples on the faces, rounded to fp32
        k = rng.integers(0, len(F), size=n)
        w = rng.dirichlet(np.ones(3), size=n)
        clouds.append((w[:, :, None] * V.astype(np.float64)[F[k]]).sum(axis=1).astype(np.float32))
        d = rng.normal(size=3)
        views.append(V.mean(axis=0) + 2.0 * d / np.linalg.norm(d))
    run = lambda: R.visible_points(clouds, meshes, views, EPS)
    tris = [torch.from_numpy(V.astype(np.float64)[F]).to(dev) for V, F in meshes]
    Pd = [torch.from_numpy(c).to(dev).double() for c in clouds]
    Cd = [torch.from_numpy(np.asarray(v)).to(dev) for v in views]
    comp = lambda: [torch_hits(C.expand_as(P).contiguous(), P - C, tri, 0.0, 1.0 - EPS, a.pairs)[2] == 0 for P, C, tri in zip(Pd, Cd, tris)]
    got, want = run(), comp()
    out = {"bench": "raycast", "shape": "visible", "meshes": M, "samples_per_mesh": n, "faces_per_mesh": VISIBLE_FACES, "eps": EPS,
           "reps": a.reps, "torch_pairs_per_step": a.pairs,
           "samples_that_differ_from_torch": int(sum(int((g != w).sum()) for g, w in zip(got, want))),
           "visible_share": round(float(torch.cat(got).double().mean()), 4),
           "wall_ms_median_min_max": BL.median_ms(run, a.reps), "kernel_ms": kernels(run, dev),
           "torch_wall_ms_median_min_max": BL.median_ms(comp, a.reps), "device": torch.cuda.get_device_name(0)}
    return rates(out, M * n * VISIBLE_FACES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1 << 24)
    ap.add_argument("--shapes", nargs="+", default=["rays", "visible"])
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "raycast_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "raycast_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    dev = torch.device("cuda")
    for shape in a.shapes:
        BL.emit({"rays": bench_rays, "visible": bench_visible}[shape](a, torch, dev), a.out)


if __name__ == "__main__":
    main()
