#!/usr/bin/env python3
"""Wall and kernel time of training-view rendering on a synthetic split: dpc.render.render_mesh_views on --models
height-field meshes with 5 views each at S = 128, ss = 3.  Appends one JSON line to --out and prints it.

    python tools/bench_mesh_render.py [--models 64] [--views 5] [--faces 2000 20000 200000] [--image-size 128]
                                      [--supersample 3] [--reps 5] [--oracle-views 2] [--out profiles/mesh_render_bench.jsonl]

ASSUMED face counts: the models' face counts cycle through --faces (2 000, 20 000 and 200 000 by default); real ShapeNet
counts have not been measured here.  render_ms: render_mesh_views from host arrays to a device synchronise, after a
warm-up, over --reps repeats (median, min, max).  kernel_ms: the library's own event timing of one call, per kernel.
tool_s: render_training_views in batches of 64 models with every view written as render_N.png / depth_N.png into a
temporary directory, one run.  oracle_s_per_view: the numpy oracle of tests/mesh_render_oracle.py on --oracle-views views
of the first models, per view, on the host that runs the benchmark.  Blender itself cannot be timed here (none is
installed): no comparison with it is made."""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np
import torch

import dpc.render as R
import mesh_render_oracle as O
from dpc.render import _native


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=64)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--faces", type=int, nargs="+", default=[2000, 20000, 200000])
    ap.add_argument("--image-size", type=int, default=128)
    ap.add_argument("--supersample", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-views", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "mesh_render_bench.jsonl"))
    a = ap.parse_args()
    kd = np.array([[0.3, 0.3, 0.9], [0.9, 0.9, 0.2]])
    scenes = [O.grid_mesh(max(1, int(round((a.faces[i % len(a.faces)] / 2) ** 0.5))), seed=i) + (kd,) for i in range(a.models)]
    faces = [len(s[1]) for s in scenes]
    pos = R.sample_camera_positions(a.models, a.views, 0)
    dev = torch.device("cuda")
    S, ss = a.image_size, a.supersample
    R.render_mesh_views(scenes[:2], pos[:2], image_size=32)  # warm-up: code object, allocator
    run = lambda: R.render_mesh_views(scenes, pos, image_size=S, supersample=ss)
    times = BL.walls_ms(run, a.reps)
    kernels = {k: float(np.sum(v)) for k, v in _native.profile_kernels(run, dev).items()}
    names = ["m%03d" % i for i in range(a.models)]
    with tempfile.TemporaryDirectory() as tmp:
        def save(name, rgba, depth, cam):
            for k in range(len(cam)):
                R.write_png_rgba(os.path.join(tmp, "%s_render_%d.png" % (name, k)), rgba[k])
                R.write_png_gray16(os.path.join(tmp, "%s_depth_%d.png" % (name, k)), depth[k])

        t0 = time.perf_counter()
        R.render_training_views(names, lambda n: scenes[int(n[1:])], pos, save, keep=False, image_size=S, supersample=ss)
        tool_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(a.oracle_views):
        O.render(*scenes[i % a.models], R.view_rotation(pos[i % a.models, 0]), 2.0, 1.875, S, ss)
    oracle_s = (time.perf_counter() - t0) / max(1, a.oracle_views)
    line = dict(tool="bench_mesh_render", models=a.models, views_per_model=a.views, faces_assumed=a.faces,
                faces_total=int(sum(faces)), image_size=S, supersample=ss, render_ms_median=float(np.median(times)),
                render_ms_min=min(times), render_ms_max=max(times), reps=a.reps,
                views_per_s=a.models * a.views / (np.median(times) / 1e3), kernel_ms=kernels, tool_s=tool_s,
                oracle_s_per_view=oracle_s, oracle_views=a.oracle_views, device=torch.cuda.get_device_name(dev))
    BL.emit(line, a.out)


if __name__ == "__main__":
    main()
