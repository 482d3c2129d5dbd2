#!/usr/bin/env python3
"""Time of closest_points_on_meshes (dpc.render.closest, csrc/dpc_closest.hip) against point_mesh_distance of the same
build, on the workloads of tools/bench_point_mesh.py (synthetic icospheres and triangle soups, uniform points).

Per (kind, faces), for the batch (--models x --views rows of --points points, one call) and for a single view (32 point
blocks, so the face range is split into chunks and the epilogue reduces several slots per point):

    distance   point_mesh_distance: wall time (packing and upload included) and the library's launch record (k_pm_*)
    closest    closest_points_on_meshes with normals: the same two figures (k_pc_* and the shared k_pm_scan), and the
               ratios closest / distance of the wall times and of the main kernels k_pc_arg / k_pm_dist
    loss       point_surface_loss on device clouds that require grad: forward alone, and forward + backward

The estimate the ratio is held against: k_pc_arg does pm_d2's FLOPS_PER_TEST - 3 = 80 operations per (point, face) plus one
compare and two selects, so about 83 / 80 of k_pm_dist, plus the epilogue (one lane per point, one face staged again).  The
squared distances of the two calls are compared bit for bit before anything is timed.  One JSON line per (kind, faces),
appended to profiles/closest_points_bench.jsonl (--out).

    python tools/bench_closest_points.py [--models 64] [--views 5] [--points 8000] [--faces 1000 20000] [--reps 3]
    python tools/bench_closest_points.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np

import bench_point_mesh as PM

FLOPS_PER_TEST = PM.FLOPS_PER_TEST + 3      # pm_d2 and, in place of the running min, one compare and two selects
mesh = PM.mesh


def resource_usage(path):
    BL.resource_usage("dpc_closest.hip", path, [
        "# k_pc_arg<fp64 points, fp64 vertices>: lds= is the face tile, DPC_PM_FACE_TILE records of 12 double2 (static);",
        "# k_pc_finish: one lane per output point, the winning face's record in registers"])


def measure(clouds, meshes, mesh_of, reps, torch, dev):
    import dpc.render as R

    dist = lambda: R.point_mesh_distance(clouds, meshes, mesh_of, squared=True)
    close = lambda: R.closest_points_on_meshes(clouds, meshes, mesh_of, normals=True)
    a, b = dist(), close()
    assert all(torch.equal(x, y.d2) for x, y in zip(a, b))                  # the same squared distances, bit for bit
    out = {"tests": int(sum(len(clouds[i]) * len(meshes[k][1]) for i, k in enumerate(mesh_of))), "rows": len(clouds),
           "distance_wall_ms_median_min_max": BL.median_ms(dist, reps), "closest_wall_ms_median_min_max": BL.median_ms(close, reps),
           "distance_kernel_ms": BL.kernel_ms(dist, dev, "k_pm_"), "closest_kernel_ms": BL.kernel_ms(close, dev, ("k_pc_", "k_pm_scan"))}
    out["wall_ratio_closest_over_distance"] = round(out["closest_wall_ms_median_min_max"][0] / out["distance_wall_ms_median_min_max"][0], 4)
    out["kernel_ratio_k_pc_arg_over_k_pm_dist"] = round(out["closest_kernel_ms"]["k_pc_arg"] / out["distance_kernel_ms"]["k_pm_dist"], 4)
    out["kernel_ratio_all_k_pc_over_all_k_pm"] = round(sum(out["closest_kernel_ms"].values()) / sum(out["distance_kernel_ms"].values()), 4)
    dev_clouds = [torch.from_numpy(c).to(dev).requires_grad_(True) for c in clouds]
    out["loss_forward_ms_median_min_max"] = BL.median_ms(lambda: R.point_surface_loss(dev_clouds, meshes, mesh_of), reps)
    out["loss_forward_backward_ms_median_min_max"] = BL.median_ms(lambda: R.point_surface_loss(dev_clouds, meshes, mesh_of).sum().backward(), reps)
    return out


def bench(a, kind, faces, torch, dev):
    rng = np.random.default_rng(5)
    meshes = [mesh(kind, faces, 100 + m) for m in range(a.models)]
    pts = (rng.random((a.models * a.views, a.points, 3)) - 0.5).astype(np.float32)
    mesh_of = [m for m in range(a.models) for _ in range(a.views)]
    return {"bench": "closest_points", "kind": kind, "faces_per_mesh": len(meshes[0][1]), "models": a.models, "views": a.views,
            "points": a.points, "reps": a.reps, "flops_per_test": FLOPS_PER_TEST, "estimated_kernel_ratio": round(FLOPS_PER_TEST / PM.FLOPS_PER_TEST, 4),
            "batch": measure(list(pts), meshes, mesh_of, a.reps, torch, dev),
            "single_view": measure([pts[0]], meshes[:1], [0], a.reps, torch, dev), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=64)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--faces", type=int, nargs="+", default=[1000, 20000])
    ap.add_argument("--kinds", nargs="+", default=["icosphere", "soup"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "closest_points_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "closest_points_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    dev = torch.device("cuda")
    for kind in a.kinds:
        for faces in a.faces:
            BL.emit(bench(a, kind, faces, torch, dev), a.out)


if __name__ == "__main__":
    main()
