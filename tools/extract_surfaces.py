#!/usr/bin/env python3
"""Turn saved predictions into triangle meshes on the GPU: one Wavefront OBJ per model.

    python tools/extract_surfaces.py --inp_dir=pred --out_dir=meshes [--vox_size=64] [--sigma_rel=1.5] [--iso_level=0.1]
                                     [--view=0] [--index_units] [--models_per_call=32]

Reads every <model>_pc.pkl of --inp_dir (load_predictions: the cloud of --view, truncated to its num_points) and every
<model>.npy (a [D,H,W] grid, singleton dimensions squeezed).  A cloud becomes a Gaussian occupancy grid first
(pointcloud2voxels at sigma = --sigma_rel / --vox_size, the exact renderer of pc_fast: false); the surface is extracted at
--iso_level (the reference's notebooks use vox_marching_cubes_isosurface = 0.1).  Both run on the GPU in batches:
--models_per_call models share an extraction call, and those of them whose clouds have the same number of points share a
pointcloud2voxels call (clouds of different lengths cannot be stacked).

Frames.  A grid from a .npy file is written in the unit cube: column c -> V_c / (G_c - 1) - 0.5, the node grid of voxelise.
pointcloud2voxels spans [-1, 1]^3 with its axes following (y, x, z) of the points; the tool swaps the first two grid axes
back before extracting, so column c follows point column c, and writes 2 * (V_c / (G_c - 1) - 0.5): the mesh of a cloud
is in the cloud's own coordinates and overlays it.  --index_units keeps node indices in both cases (for a cloud, of the
grid with its axes swapped back).  Writes <out_dir>/<model>.obj and skips models whose output already exists."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-unsup-pc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def parse_arguments(argv):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--inp_dir", type=str, required=True)
    parser.add_argument("--out_dir", type=str, required=True)
    parser.add_argument("--vox_size", type=int, default=64)
    parser.add_argument("--sigma_rel", type=float, default=1.5)
    parser.add_argument("--iso_level", type=float, default=0.1)
    parser.add_argument("--view", type=int, default=0)
    parser.add_argument("--index_units", action="store_true")
    parser.add_argument("--models_per_call", type=int, default=32)
    return parser.parse_args(argv)


class _Cfg:
    def __init__(self, vox_size):
        self.vox_size = vox_size


def main(argv=None):
    """Returns {"written": [names], "skipped": [names]}."""
    import numpy as np
    import torch

    from dpc.render import extract_surfaces, load_predictions, pointcloud2voxels, save_obj

    cfg = parse_arguments(sys.argv[1:] if argv is None else argv)
    if cfg.models_per_call < 1:
        raise SystemExit("extract_surfaces.py: --models_per_call must be >= 1")
    os.makedirs(cfg.out_dir, exist_ok=True)
    items = []
    for f in sorted(os.listdir(cfg.inp_dir)):
        if f.endswith("_pc.pkl"):
            items.append((f[:-len("_pc.pkl")], "cloud", os.path.join(cfg.inp_dir, f)))
        elif f.endswith(".npy"):
            items.append((f[:-len(".npy")], "grid", os.path.join(cfg.inp_dir, f)))
    out_path = lambda name: os.path.join(cfg.out_dir, "%s.obj" % name)
    skipped = [n for n, _, _ in items if os.path.isfile(out_path(n))]
    todo = [it for it in items if not os.path.isfile(out_path(it[0]))]
    dev = torch.device("cuda")
    written = []
    for a in range(0, len(todo), cfg.models_per_call):
        group = todo[a:a + cfg.models_per_call]
        grids, clouds = [None] * len(group), {}
        for i, (name, kind, path) in enumerate(group):
            if kind == "grid":
                grids[i] = torch.from_numpy(np.squeeze(np.load(path))).to(dev)
                continue
            points, _, nums = load_predictions(path)
            cloud = points[cfg.view] if nums is None else points[cfg.view][:int(nums[cfg.view])]
            clouds.setdefault(len(cloud), []).append((i, np.ascontiguousarray(cloud, dtype=np.float32)))
        for same in clouds.values():      # clouds of one length: one pointcloud2voxels call
            batch = torch.from_numpy(np.stack([c for _, c in same])).to(dev)
            with torch.no_grad():
                vox = pointcloud2voxels(_Cfg(cfg.vox_size), batch, cfg.sigma_rel / cfg.vox_size)[..., 0]
            vox = vox.transpose(1, 2).contiguous()      # grid axis c follows point column c again
            for (i, _), g in zip(same, vox):
                grids[i] = g
        for (name, kind, _), (V, F) in zip(group, extract_surfaces(grids, cfg.iso_level, unit_cube=not cfg.index_units)):
            if kind == "cloud" and not cfg.index_units:
                V = 2.0 * V                              # that grid spans [-1, 1]^3, not the unit cube
            save_obj(out_path(name), V, F)
            written.append(name)
            print("%d/%d %s (%d vertices, %d faces)" % (len(written), len(todo), name, len(V), len(F)))
    return {"written": written, "skipped": skipped}


if __name__ == "__main__":
    main()
