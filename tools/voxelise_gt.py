#!/usr/bin/env python3
"""Voxelise ShapeNet meshes into solid ground-truth occupancy grids on the GPU: the <model>.mat files with a `Volume`
array that the reference expects ready-made (dpc/run/create_tf_records.py:104-115), which it made off-line with binvox.

    python tools/voxelise_gt.py --shapenet_path=ShapeNetCore.v1 --synth_set=03001627 --subset=test \\
                                --output_dir=gt/voxels [--shapenet_v2] [--vox_size=32] [--fill=carve] [--models_per_call=256]

Reads the model names from splits/<synth_set>_<subset>.txt (relative to the working directory, as the reference does)
and each mesh from <shapenet_path>/<synth_set>/<model>/model.obj (models/model_normalized.obj with --shapenet_v2), every
face kept and polygons fan-triangulated (load_obj_scene).  Writes <output_dir>/<synth_set>/<model>.mat with
{"Volume": uint8 [G,G,G]} and skips models whose output already exists.  The grid is this library's: node-centred over
[-1/2, 1/2]^3, .obj column c on grid axis c, like the clouds voxelise takes -- NOT the axis frame or the bits of the
binvox files the reference downloads.  --fill: "carve" (the default; robust to ShapeNet's open meshes), "parity" or
"none" (voxelise_meshes).  A model that cannot be read is reported and skipped, and the others go on."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-unsup-pc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def parse_arguments(argv):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--shapenet_path", type=str, required=True)
    parser.add_argument("--synth_set", type=str, required=True)
    parser.add_argument("--subset", type=str, default="val")
    parser.add_argument("--output_dir", type=str, required=True)
    parser.add_argument("--shapenet_v2", action="store_true")
    parser.add_argument("--vox_size", type=int, default=32)
    parser.add_argument("--fill", type=str, default="carve", choices=("none", "carve", "parity"))
    parser.add_argument("--models_per_call", type=int, default=256)
    return parser.parse_args(argv)


def main(argv=None):
    """Returns {"written": [names], "skipped": [names], "failed": {name: message}}."""
    import numpy as np
    import scipy.io

    from dpc.render import load_obj_scene, voxelise_meshes

    cfg = parse_arguments(sys.argv[1:] if argv is None else argv)
    if cfg.models_per_call < 1:
        raise SystemExit("voxelise_gt.py: --models_per_call must be >= 1")
    with open("splits/{}_{}.txt".format(cfg.synth_set, cfg.subset)) as fh:
        models = [l.strip() for l in fh if l.strip()]
    model_file = os.path.join("models", "model_normalized.obj") if cfg.shapenet_v2 else "model.obj"
    out_dir = os.path.join(cfg.output_dir, cfg.synth_set)
    os.makedirs(out_dir, exist_ok=True)
    out_path = lambda name: os.path.join(out_dir, "%s.mat" % name)
    todo = [n for n in models if not os.path.isfile(out_path(n))]
    skipped = [n for n in models if os.path.isfile(out_path(n))]
    for n in skipped:
        print("already computed", n)
    written, failed = [], {}
    for a in range(0, len(todo), cfg.models_per_call):
        names, meshes = [], []
        for name in todo[a:a + cfg.models_per_call]:
            try:
                meshes.append(load_obj_scene(os.path.join(cfg.shapenet_path, cfg.synth_set, name, model_file))[:2])
                names.append(name)
            except (ValueError, IndexError, OSError) as exc:
                failed[name] = str(exc)
        if not names:
            continue
        grids, info = voxelise_meshes(meshes, cfg.vox_size, fill=cfg.fill, return_info=True)
        grids, info = grids.cpu().numpy().astype(np.uint8), info.cpu().numpy()
        for name, grid, (outside, opened) in zip(names, grids, info):
            scipy.io.savemat(out_path(name), {"Volume": grid})
            written.append(name)
            print("{}/{} {} ({} voxels{}{})".format(len(written), len(todo), name, int(grid.sum()),
                                                     ", %d faces reach outside the cube" % outside if outside else "",
                                                     ", %d open columns" % opened if opened else ""))
    for name, msg in failed.items():
        print("failed", name, msg)
    return {"written": written, "skipped": skipped, "failed": failed}


if __name__ == "__main__":
    main()
