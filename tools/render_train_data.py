#!/usr/bin/env python3
"""Render the training views of ShapeNet meshes on the GPU: what the reference downloads as <synth_set>-renders.tar.gz
(data/download_train_data.sh), made here from the meshes themselves.

    python tools/render_train_data.py --shapenet_path=ShapeNetCore.v1 --synth_set=03001627 --subset=train \\
                                      --out_dir=renders [--num_views=5] [--image_size=128] [--seed=0] \\
                                      [--write_features=DIR] [--shapenet_v2] [--supersample=3] [--models_per_call=64] \\
                                      [--textures] [--smooth_normals]

Reads the model names from splits/<synth_set>_<subset>.txt (relative to the working directory, as the reference does)
and each mesh from <shapenet_path>/<synth_set>/<model>/model.obj (models/model_normalized.obj with --shapenet_v2), with
the diffuse colours of its .mtl files.  Writes <out_dir>/<synth_set>/<model>/render_N.png (RGBA), depth_N.png (16 bits
over [0, 10]) and camera_N.mat ({"extrinsic", "pos"}) for N = 0 .. num_views - 1: the archive's layout, so the
reference's dpc/run/create_data_torch.py runs on it unchanged.  With --write_features it also writes
DIR/<model>_features.p itself (image, mask, name, extrinsic, cam_pos, depth at --image_size; no resize).  Camera
positions are drawn by dpc.render.sample_camera_positions from --seed and the model's place in the split (its ranges
are an assumption: the archive's are not recorded), so a rerun draws the same views.  Models whose outputs all exist are
skipped; a model that cannot be read or rendered is reported and skipped, and the others go on.  --textures uses the
models' map_Kd images where faces have texture coordinates, --smooth_normals their vn normals (both off by default: flat
facets in each material's diffuse colour); an image that cannot be read leaves its material untextured and is listed
per model under "warnings" in the summary."""
import argparse
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-unsup-pc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def parse_arguments(argv):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--shapenet_path", type=str, required=True)
    parser.add_argument("--synth_set", type=str, required=True)
    parser.add_argument("--subset", type=str, default="train")
    parser.add_argument("--out_dir", type=str, required=True)
    parser.add_argument("--num_views", type=int, default=5)
    parser.add_argument("--image_size", type=int, default=128)
    parser.add_argument("--supersample", type=int, default=3)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--write_features", type=str, default="")
    parser.add_argument("--shapenet_v2", action="store_true")
    parser.add_argument("--models_per_call", type=int, default=64)
    parser.add_argument("--camera_distance", type=float, default=2.0)
    parser.add_argument("--focal_length", type=float, default=1.875)
    parser.add_argument("--textures", action="store_true")
    parser.add_argument("--smooth_normals", action="store_true")
    return parser.parse_args(argv)


def main(argv=None):
    """Returns {"written": [names], "skipped": [names], "failed": {name: message}}, with --textures or --smooth_normals
    also "warnings": {name: [messages]} for the models whose loading left any."""
    import scipy.io

    from dpc.render import (camera_extrinsic, features_of_views, load_obj_scene, load_obj_scene_shaded,
                            render_training_views, sample_camera_positions, write_png_gray16, write_png_rgba)

    cfg = parse_arguments(sys.argv[1:] if argv is None else argv)
    if cfg.num_views < 1:
        raise SystemExit("render_train_data.py: --num_views must be >= 1")
    with open("splits/{}_{}.txt".format(cfg.synth_set, cfg.subset)) as fh:
        models = [l.strip() for l in fh if l.strip()]
    model_file = os.path.join("models", "model_normalized.obj") if cfg.shapenet_v2 else "model.obj"
    out_dir = os.path.join(cfg.out_dir, cfg.synth_set)
    os.makedirs(out_dir, exist_ok=True)
    if cfg.write_features:
        os.makedirs(cfg.write_features, exist_ok=True)

    def outputs(name):
        files = [os.path.join(out_dir, name, "%s_%d.%s" % (kind, k, ext)) for k in range(cfg.num_views)
                 for kind, ext in (("render", "png"), ("depth", "png"), ("camera", "mat"))]
        if cfg.write_features:
            files.append(os.path.join(cfg.write_features, "%s_features.p" % name))
        return files

    done = lambda name: all(os.path.isfile(f) for f in outputs(name))
    todo = [n for n in models if not done(n)]
    skipped = [n for n in models if done(n)]
    for n in skipped:
        print("already rendered", n)
    positions = sample_camera_positions(len(models), cfg.num_views, cfg.seed)   # by place in the split: stable across reruns
    cam_pos = {n: positions[i] for i, n in enumerate(models)}

    shaded = cfg.textures or cfg.smooth_normals
    warnings = {}

    def load_scene(name):
        path = os.path.join(cfg.shapenet_path, cfg.synth_set, name, model_file)
        if not shaded:
            return load_obj_scene(path)
        scene = load_obj_scene_shaded(path)
        if scene.warnings:
            warnings[name] = list(scene.warnings)
        return scene

    def save(name, rgba, depth, pos):
        os.makedirs(os.path.join(out_dir, name), exist_ok=True)
        extr = [camera_extrinsic(p, cfg.camera_distance) for p in pos]
        for k in range(len(pos)):
            write_png_rgba(os.path.join(out_dir, name, "render_%d.png" % k), rgba[k])
            write_png_gray16(os.path.join(out_dir, name, "depth_%d.png" % k), depth[k])
            scipy.io.savemat(os.path.join(out_dir, name, "camera_%d.mat" % k), {"extrinsic": extr[k], "pos": pos[k]})
        if cfg.write_features:
            feature = features_of_views(rgba, depth, pos, extr, name, image_size=cfg.image_size)
            with open(os.path.join(cfg.write_features, "%s_features.p" % name), "wb") as fh:
                pickle.dump(feature, fh)
        print("{}/{} {}".format(len(written) + 1, len(todo), name))
        written.append(name)

    written, failed = [], {}
    render_training_views(todo, load_scene, cam_pos, save, cfg.models_per_call, errors=failed, keep=False,
                          image_size=cfg.image_size, supersample=cfg.supersample, camera_distance=cfg.camera_distance,
                          focal_length=cfg.focal_length, textures=cfg.textures, smooth_normals=cfg.smooth_normals)
    for name, msg in failed.items():
        print("failed", name, msg)
    summary = {"written": written, "skipped": skipped, "failed": failed}
    if shaded:
        for name, lines in warnings.items():
            for line in lines:
                print("warning", name, line)
        summary["warnings"] = warnings
    return summary


if __name__ == "__main__":
    main()
