#!/usr/bin/env python3
"""Densify ShapeNet meshes into dense ground-truth clouds on the GPU: the reference's densify/densify.py plus
densify_single.py (run by data/generate_ground_truth.sh), executed here instead of written out as a list of commands.

    python tools/densify_gt.py --shapenet_path=ShapeNetCore.v1 --synth_set=03001627 --subset=test \\
                               --output_dir=gt/dense [--shapenet_v2] [--num_points=100000] [--models_per_call=256]

Reads the model names from splits/<synth_set>_<subset>.txt (relative to the working directory, as the reference does)
and each mesh from <shapenet_path>/<synth_set>/<model>/model.obj (models/model_normalized.obj with --shapenet_v2).
Writes <output_dir>/<synth_set>/<model>.mat with {"points": the parsed vertices, then num_points midpoints} and, as the
reference does, skips models whose output already exists.  Every point equals the reference's, in its order, bit for bit.
A model that cannot be read or densified is reported and skipped, as a failed command of the reference would be, and
the others go on.  --num_points must be >= 1 (the reference's V[-0:] would save the vertices twice)."""
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
    parser.add_argument("--num_points", type=int, default=100000)
    parser.add_argument("--models_per_call", type=int, default=256)
    return parser.parse_args(argv)


def main(argv=None):
    """Returns {"written": [names], "skipped": [names], "failed": {name: message}}."""
    import scipy.io

    from dpc.render import densify_split, load_obj_mesh

    cfg = parse_arguments(sys.argv[1:] if argv is None else argv)
    if cfg.num_points < 1:
        raise SystemExit("densify_gt.py: --num_points must be >= 1")
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

    def load_mesh(name):
        return load_obj_mesh(os.path.join(cfg.shapenet_path, cfg.synth_set, name, model_file))

    def save(name, points):
        scipy.io.savemat(out_path(name), {"points": points})
        print("{}/{} {}".format(len(written) + 1, len(todo), name))
        written.append(name)

    written, failed = [], {}
    densify_split(todo, load_mesh, cfg.num_points, save, cfg.models_per_call, errors=failed, keep=False)
    for name, msg in failed.items():
        print("failed", name, msg)
    return {"written": written, "skipped": skipped, "failed": failed}


if __name__ == "__main__":
    main()
