#!/usr/bin/env python3
"""Time of the generalized winding numbers (dpc.render.winding, csrc/dpc_winding.hip) against the same formula composed
from torch ops on the same device, at two shapes:

    points   winding_numbers of 100 000 fp32 query points about one mesh of 20 000 faces
    voxels   winding_voxels (surface=False) of 32 meshes at 32^3

Per shape: the wall time of the Python call (packing and upload included), the library's launch record (k_wn_*, k_pm_scan),
the (point, face) pairs per second of the wall time and of the kernels, and the composition's wall time -- torch_sums
below, the rule of include/dpc_render.h (dpc_mesh_winding) in fp64 torch ops, at most --pairs (point, face) pairs at a
time so that its [P,F,3] temporaries fit.  The composition's int64 sums are compared with the kernel's before anything
is timed: they may differ by one quantum per face (tests/winding_oracle.py), and the grids must be equal.  One JSON line
per shape, appended to profiles/winding_bench.jsonl (--out).

    python tools/bench_winding.py [--reps 3] [--pairs 16777216]
    python tools/bench_winding.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np

POINTS_SHAPE = (100000, 20000)      # query points, faces
VOXELS_SHAPE = (32, 32)             # meshes, grid side
VOXEL_FACES = 1280


def resource_usage(path):
    BL.resource_usage("dpc_winding.hip", path, [
        "# k_wn_sum<fp64 points, fp64 vertices>, k_wn_vox<fp64 vertices>: lds= is the face tile, DPC_PM_FACE_TILE records of",
        "# 5 double2 (static); k_wn_finish, k_wn_vox_finish: one lane per output point / node"])


def mesh(faces, seed=0):
    """(V fp32 [n,3], F int32 [faces,3]): the first `faces` faces of the smallest icosphere that has as many (a sphere
    with a hole when it has more), scaled and moved a little by the seed."""
    import mesh_voxels_oracle as MV

    V, F = MV.icosphere(max(0, int(np.ceil(np.log(faces / 20.0) / np.log(4.0)))), 1.0)
    rng = np.random.default_rng(seed)
    return (V * (0.36 + 0.08 * rng.random()) + (rng.random(3) - 0.5) * 0.08).astype(np.float32), np.ascontiguousarray(F[:faces], dtype=np.int32)


def torch_sums(P, tri, pairs):
    """The int64 winding sums [n] of P [n,3] fp64 about the triangles tri [f,3,3] fp64 on the device, from torch ops, at
    most `pairs` (point, face) pairs at a time."""
    import torch

    out = torch.empty((len(P),), dtype=torch.int64, device=P.device)
    step = max(1, pairs // max(1, len(tri)))
    dot = lambda x, y: (x * y).sum(-1)
    for s in range(0, len(P), step):
        p = P[s:s + step, None, :]
        a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        det = dot(a, torch.cross(b, c, dim=-1))
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
        t = torch.where(det == 0, torch.zeros_like(det), torch.atan2(det, den) / (2.0 * np.pi))
        out[s:s + step] = torch.round(t * 2.0 ** 40).to(torch.int64).sum(1)
    return out


def kernels(fn, dev):
    return BL.kernel_ms(fn, dev, ("k_wn_", "k_pm_scan"))


def rates(out, pairs):
    out["pairs"] = int(pairs)
    out["kernel_ms_total"] = round(sum(out["kernel_ms"].values()), 4)
    out["gpairs_per_s_wall"] = round(pairs / out["wall_ms_median_min_max"][0] * 1e-6, 3)
    out["gpairs_per_s_kernel"] = round(pairs / out["kernel_ms_total"] * 1e-6, 3)
    out["torch_over_wall"] = round(out["torch_wall_ms_median_min_max"][0] / out["wall_ms_median_min_max"][0], 3)
    return out


def bench_points(a, torch, dev):
    import dpc.render as R

    n, f = POINTS_SHAPE
    V, F = mesh(f)
    P = (np.random.default_rng(5).random((n, 3)) - 0.5).astype(np.float32)
    run = lambda: R.winding_numbers([P], [(V, F)], return_sums=True)
    Pd = torch.from_numpy(P).to(dev).double()
    tri = torch.from_numpy(V.astype(np.float64)[F]).to(dev)
    comp = lambda: torch_sums(Pd, tri, a.pairs)
    diff = int((run()[1][0] - comp()).abs().max())
    assert diff <= f, diff
    out = {"bench": "winding", "shape": "points", "points": n, "faces": f, "reps": a.reps, "torch_pairs_per_step": a.pairs,
           "max_quanta_kernel_minus_torch": diff, "wall_ms_median_min_max": BL.median_ms(run, a.reps), "kernel_ms": kernels(run, dev),
           "torch_wall_ms_median_min_max": BL.median_ms(comp, a.reps), "device": torch.cuda.get_device_name(0)}
    return rates(out, n * f)


def bench_voxels(a, torch, dev):
    import dpc.render as R
    import winding_oracle as WO

    M, G = VOXELS_SHAPE
    meshes = [mesh(VOXEL_FACES, 100 + m) for m in range(M)]
    run = lambda: R.winding_voxels(meshes, G, surface=False)
    nodes = torch.from_numpy(WO.node_centres((G, G, G))).to(dev)
    tris = [torch.from_numpy(V.astype(np.float64)[F]).to(dev) for V, F in meshes]
    half = WO.threshold_q(0.5)
    comp = lambda: torch.stack([(torch_sums(nodes, tri, a.pairs) > half).reshape(G, G, G) for tri in tris])
    got, want = run(), comp()
    differ = int((got != want).sum())           # a node within a few quanta of the threshold may differ; none does here
    out = {"bench": "winding", "shape": "voxels", "meshes": M, "side": G, "faces_per_mesh": VOXEL_FACES, "reps": a.reps,
           "torch_pairs_per_step": a.pairs, "nodes_that_differ_from_torch": differ, "occupied": int(got.sum()),
           "wall_ms_median_min_max": BL.median_ms(run, a.reps), "kernel_ms": kernels(run, dev),
           "torch_wall_ms_median_min_max": BL.median_ms(comp, a.reps), "device": torch.cuda.get_device_name(0)}
    return rates(out, M * G ** 3 * VOXEL_FACES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1 << 24)
    ap.add_argument("--shapes", nargs="+", default=["points", "voxels"])
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "winding_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "winding_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    dev = torch.device("cuda")
    for shape in a.shapes:
        BL.emit({"points": bench_points, "voxels": bench_voxels}[shape](a, torch, dev), a.out)


if __name__ == "__main__":
    main()
