#!/usr/bin/env python3
"""Downsample dense ground-truth clouds on the GPU: the reference's densify/downsample_gt.py (run by
data/downsample_ground_truth.sh) without open3d.

    python tools/downsample_gt.py --inp_dir=gt/dense --out_dir=gt/downsampled --synth_set=03001627 \\
                                  [--downsample_voxel_size=0.01] [--clouds_per_call=256]

Reads <inp_dir>/<synth_set>/*.mat (key "points"), writes <out_dir>/<synth_set>/<name>.mat (key "points", float64) and, as
the reference does, skips models whose output already exists.  Every output point equals open3d's voxel_down_sample bit
for bit; the voxels come in ascending (kx, ky, kz) order instead of open3d's hash-map order."""
import argparse
import glob
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
    parser.add_argument("--synth_set", type=str, default="03001627")
    parser.add_argument("--downsample_voxel_size", type=float, default=0.01)
    parser.add_argument("--clouds_per_call", type=int, default=256)
    return parser.parse_args(argv)


def main(argv=None):
    """Returns {"written": [names], "skipped": [names]}."""
    import scipy.io

    from dpc.render import downsample_split

    cfg = parse_arguments(sys.argv[1:] if argv is None else argv)
    inp_dir = os.path.join(cfg.inp_dir, cfg.synth_set)
    out_dir = os.path.join(cfg.out_dir, cfg.synth_set)
    os.makedirs(out_dir, exist_ok=True)
    names = sorted(os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(inp_dir, "*.mat")))
    out_path = lambda name: os.path.join(out_dir, "%s.mat" % name)
    todo = [n for n in names if not os.path.isfile(out_path(n))]
    skipped = [n for n in names if os.path.isfile(out_path(n))]
    for n in skipped:
        print("already exists:", n)

    def load_dense(name):
        return scipy.io.loadmat(os.path.join(inp_dir, "%s.mat" % name))["points"]

    def save(name, points):
        scipy.io.savemat(out_path(name), {"points": points})
        print("{}/{} {}".format(len(written) + 1, len(todo), name))
        written.append(name)

    written = []
    downsample_split(todo, load_dense, cfg.downsample_voxel_size, save, cfg.clouds_per_call)
    return {"written": written, "skipped": skipped}


if __name__ == "__main__":
    main()
