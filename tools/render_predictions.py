#!/usr/bin/env python3
"""Render predicted point clouds to PNG images on the GPU: the reference's dpc/render/render_point_cloud_runner.py (one
Blender process per model) without Blender.

    python tools/render_predictions.py --inp_dir=<exp>/<save_predictions_dir> --out_dir=<exp>/render \\
        [--models_list=names.txt] [--vis_azimuth=140] [--vis_elevation=15] [--vis_dist=2] [--render_image_size=256] \\
        [--supersample=3] [--like_train_data] [--models_per_call=256] [--voxels] [--vis_threshold=0.5]

Per model, the first existing file of <inp_dir>/<model>_pc.mat (key "points"), <model>_pc.npz ("arr_0") and
<model>_pc.pkl (dpc.render.load_predictions) is read, view 0 rendered and written to <out_dir>/<model>.png; images that
already exist are skipped ("already rendered").  A model with no prediction file is an error naming it.  Without
--models_list every *_pc.{mat,npz,pkl} of inp_dir is rendered.  The runner does not pass like_train_data, so Blender's
startup camera (35 mm) applies there: --lens_mm defaults to 35, --like_train_data sets 60.

With --voxels (the Blender script's --voxels mode, render_point_cloud_blender.py:199-227) the inputs are
<inp_dir>/<model>_vox.npz: key "arr_0", the first view, squeezed to a cubic grid; the voxels above --vis_threshold are
drawn as points of size 0.01 at the places voxel2pc gives them (dpc.render.render_voxels)."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-unsup-pc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SUFFIXES = ("_pc.mat", "_pc.npz", "_pc.pkl")
VOXEL_SUFFIX = "_vox.npz"
VOXEL_POINT_SIZE = 0.01   # load_voxels' DEFAULT_SIZE


def parse_arguments(argv):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--inp_dir", type=str, required=True)
    parser.add_argument("--out_dir", type=str, required=True)
    parser.add_argument("--models_list", type=str, default="")
    parser.add_argument("--vis_azimuth", type=float, default=140.0)
    parser.add_argument("--vis_elevation", type=float, default=15.0)
    parser.add_argument("--vis_dist", type=float, default=2.0)
    parser.add_argument("--render_image_size", type=int, default=256)
    parser.add_argument("--supersample", type=int, default=3)
    parser.add_argument("--lens_mm", type=float, default=35.0)
    parser.add_argument("--like_train_data", action="store_true")
    parser.add_argument("--models_per_call", type=int, default=256)
    parser.add_argument("--voxels", action="store_true")
    parser.add_argument("--vis_threshold", type=float, default=0.5)
    return parser.parse_args(argv)


def prediction_file(inp_dir, name):
    """The first existing <name>_pc.{mat,npz,pkl}; AssertionError naming the model when there is none."""
    for suffix in SUFFIXES:
        path = os.path.join(inp_dir, name + suffix)
        if os.path.isfile(path):
            return path
    raise AssertionError("no input file with saved point cloud for model %r in %s" % (name, inp_dir))


def load_points(path):
    if path.endswith(".mat"):
        import scipy.io

        return scipy.io.loadmat(path)["points"]
    if path.endswith(".npz"):
        import numpy as np

        return np.load(path)["arr_0"]
    from dpc.render import load_predictions

    return load_predictions(path)[0]


def load_voxels(path):
    """load_voxels of the Blender script: "arr_0" of the file, the first view, squeezed."""
    import numpy as np

    return np.squeeze(np.load(path)["arr_0"][0])


def render_voxel_files(cfg):
    """The --voxels mode: one render_voxels call per <model>_vox.npz."""
    from dpc.render import render_voxels, write_png

    if cfg.models_list:
        with open(cfg.models_list) as fh:
            names = [line.strip() for line in fh if line.strip()]
    else:
        names = sorted(os.path.basename(f)[:-len(VOXEL_SUFFIX)] for f in glob.glob(os.path.join(cfg.inp_dir, "*" + VOXEL_SUFFIX)))
    os.makedirs(cfg.out_dir, exist_ok=True)
    out_path = lambda name: os.path.join(cfg.out_dir, "%s.png" % name)
    skipped = [n for n in names if os.path.isfile(out_path(n))]
    for n in skipped:
        print("{} already rendered".format(n))
    todo = [n for n in names if not os.path.isfile(out_path(n))]
    for n in todo:
        if not os.path.isfile(os.path.join(cfg.inp_dir, n + VOXEL_SUFFIX)):
            raise AssertionError("no input file with saved voxels for model %r in %s" % (n, cfg.inp_dir))
    for n in todo:
        image = render_voxels(load_voxels(os.path.join(cfg.inp_dir, n + VOXEL_SUFFIX)), cfg.vis_threshold, azimuth=cfg.vis_azimuth,
                              elevation=cfg.vis_elevation, dist=cfg.vis_dist, image_size=cfg.render_image_size,
                              supersample=cfg.supersample, lens_mm=60.0 if cfg.like_train_data else cfg.lens_mm,
                              point_size=VOXEL_POINT_SIZE)
        write_png(out_path(n), image)
    return {"written": todo, "skipped": skipped}


def main(argv=None):
    """Returns {"written": [names], "skipped": [names]}."""
    from dpc.render import render_split, write_png

    cfg = parse_arguments(sys.argv[1:] if argv is None else argv)
    if cfg.voxels:
        return render_voxel_files(cfg)
    if cfg.models_list:
        with open(cfg.models_list) as fh:
            names = [line.strip() for line in fh if line.strip()]
    else:
        found = set()
        for suffix in SUFFIXES:
            found.update(os.path.basename(f)[:-len(suffix)] for f in glob.glob(os.path.join(cfg.inp_dir, "*" + suffix)))
        names = sorted(found)
    os.makedirs(cfg.out_dir, exist_ok=True)
    out_path = lambda name: os.path.join(cfg.out_dir, "%s.png" % name)
    skipped = [n for n in names if os.path.isfile(out_path(n))]
    for n in skipped:
        print("{} already rendered".format(n))
    todo = [n for n in names if not os.path.isfile(out_path(n))]
    files = {n: prediction_file(cfg.inp_dir, n) for n in todo}  # every missing file is an error before any rendering

    written = []

    def save(name, image):
        write_png(out_path(name), image)
        written.append(name)

    render_split(todo, lambda n: load_points(files[n]), save, models_per_call=cfg.models_per_call,
                 azimuth=cfg.vis_azimuth, elevation=cfg.vis_elevation, dist=cfg.vis_dist, image_size=cfg.render_image_size,
                 supersample=cfg.supersample, lens_mm=60.0 if cfg.like_train_data else cfg.lens_mm)
    return {"written": written, "skipped": skipped}


if __name__ == "__main__":
    main()
