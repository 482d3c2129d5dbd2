#!/usr/bin/env python3
"""Time of the iso-surface extraction (dpc.render.surface, csrc/dpc_surface.hip): --grids grids of 64^3 made by
pointcloud2voxels (Gaussian occupancy, level 0.1) and of 128^3 made by voxelise (bool occupancy, level 0.5), both from
seeded clouds on a bumpy sphere.

Per shape one JSON line, appended to profiles/surface_bench.jsonl (--out): the wall time of extract_surfaces (count call,
the read of the counts, extract call), the kernel times from the library's launch record, the bytes each kernel must move
(computed from the shapes and the counts) over its time as a share of the HBM peak (8.0 TB/s), and the numpy oracle's
(tests/surface_oracle.py) time on the host for --host-items grids, scaled to the batch.  The meshes are compared with the
oracle's for those grids before anything is timed.  There is no pass mark: nothing earlier exists to compare against.

    python tools/bench_surface.py [--grids 32] [--reps 20] [--host-items 2] [--out FILE]
    python tools/bench_surface.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np

TILE = 1024         # nodes of a workgroup (csrc/dpc_surface.hip)


def resource_usage(path):
    BL.resource_usage("dpc_surface.hip", path, [
        "# k_surface_tiles<fp64 input>, k_surface_verts<fp64 input>; all LDS is static"])


def clouds(B, n, seed):
    """[B,n,3] float32 points on bumpy spheres inside [-0.4, 0.4]^3."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(B, n, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    r = 0.3 + 0.06 * np.sin(5.0 * d[..., :1] + rng.random((B, 1, 1)) * 6.0) * np.cos(4.0 * d[..., 1:2])
    return (d * r).astype(np.float32)


class _Cfg:
    def __init__(self, vox_size):
        self.vox_size = vox_size


def bench(a, G, torch, R, O, dev):
    B = a.grids
    if G <= 64:
        pts = torch.from_numpy(clouds(B, 8000, G)).to(dev)
        with torch.no_grad():
            grids = R.pointcloud2voxels(_Cfg(G), pts * 2.0, 1.5 / G)[..., 0].contiguous()   # that grid spans [-1, 1]^3
        iso, source = 0.1, "pointcloud2voxels(8000 points, sigma 1.5 / G)"
    else:
        pts = torch.from_numpy(clouds(B, 200000, G)).to(dev)
        grids = R.voxelise(pts, G).to(torch.float32)
        iso, source = 0.5, "voxelise(200000 points)"
    run = lambda: R.extract_surfaces(grids, iso)
    meshes = run()
    nv, nf = sum(len(v) for v, _ in meshes), sum(len(f) for _, f in meshes)
    k = min(a.host_items, B)
    host = grids[:k].cpu().numpy()
    t0 = time.perf_counter()
    for i in range(k):
        verts, faces, _ = O.extract(host[i], iso)
        assert np.array_equal(meshes[i][0].cpu().numpy(), verts) and np.array_equal(meshes[i][1].cpu().numpy(), faces), "differs from the oracle"
    host_ms = (time.perf_counter() - t0) * 1e3 / max(k, 1)
    assert R.check_status() == 0
    wall = BL.walls_ms(run, a.reps, warmup=0)         # run() above was the warm-up call
    km = BL.kernel_ms(run, dev, "k_surface")
    nodes, tiles = B * G ** 3, B * -(-G ** 3 // TILE)
    # what each kernel must move: tiles and scan run in both calls; the map is one int32 a node
    nbytes = {"k_surface_tiles": 2 * (nodes * 4 + tiles * 8), "k_surface_scan": 2 * (2 * tiles * 8),
              "k_surface_verts": nodes * 4 + nodes * 4 + nv * 24, "k_surface_faces": nodes * 4 + nf * 12}
    return {
        "bench": "surface", "measured_on": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]), "grid": G, "grids": B, "source": source, "iso_level": iso,
        "vertices": nv, "faces": nf, "reps": a.reps,
        "wall_ms_median_min_max": BL.stats(wall),
        "kernel_ms": km, "kernel_bytes": nbytes,
        "kernel_share_of_hbm_peak": {n: BL.share(b, km.get(n), BL.HBM_PEAK, 4) for n, b in nbytes.items()},
        "numpy_grids_timed": k, "numpy_host_ms_per_grid": round(host_ms, 1), "numpy_host_ms_scaled_to_batch": round(host_ms * B, 1),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-items", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "surface_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "surface_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    import dpc.render as R
    import surface_oracle as O

    dev = torch.device("cuda")
    for G in (64, 128):
        BL.emit(bench(a, G, torch, R, O, dev), a.out)


if __name__ == "__main__":
    main()
