#!/usr/bin/env python3
"""Wall time of point-cloud rendering at the chair test split's shape: dpc.render.render_point_clouds on 1 356 clouds of
8 000 tanh-distributed points (float32, like the predictions), ss = 3, at S = 256 (render_image_size) and 512 (the
notebooks).  Appends one JSON line per size to --out and prints it.

    python tools/bench_render.py [--clouds 1356] [--points 8000] [--sizes 256 512] [--supersample 3] [--reps 5]
                                 [--oracle-images 2] [--out profiles/render_bench.jsonl]

render_ms: render_point_clouds (uint8 images left on the device) from host clouds to a device synchronise, after a
warm-up, over --reps repeats (median, min, max).  tool_s: the runner end to end as tools/render_predictions.py does it
(render_split in batches of 256, every image copied to the host and written as a PNG into a temporary directory), one
run.  oracle_s_per_image: the numpy oracle of tests/render_oracle.py on --oracle-images images, per image, on the host
that runs the benchmark.  Blender itself cannot be timed here (none is installed): no comparison with it is made."""
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
import render_oracle as O
from dpc.render import visualise as V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1356)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--supersample", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-images", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "render_bench.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    clouds = [(np.tanh(rng.standard_normal((a.points, 3))) * 0.5).astype(np.float32) for _ in range(a.clouds)]
    dev = torch.device("cuda")
    R.render_point_clouds(clouds[:2], image_size=64)  # warm-up: code object, allocator
    for S in a.sizes:
        run = lambda: R.render_point_clouds(clouds, image_size=S, supersample=a.supersample)
        times = BL.walls_ms(run, a.reps)
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            R.render_split(list(range(a.clouds)), lambda i: clouds[i][None],
                           save=lambda i, img: V.write_png(os.path.join(tmp, "%d.png" % i), img), image_size=S,
                           supersample=a.supersample)
            tool_s = time.perf_counter() - t0
        frame = V.camera_frame(140.0, 15.0, 2.0)
        t0 = time.perf_counter()
        for i in range(a.oracle_images):
            O.render(clouds[i], frame, S, a.supersample, 1.875 * S)
        oracle_s = (time.perf_counter() - t0) / max(1, a.oracle_images)
        line = dict(tool="bench_render", clouds=a.clouds, points=a.points, image_size=S, supersample=a.supersample,
                    render_ms_median=float(np.median(times)), render_ms_min=min(times), render_ms_max=max(times),
                    reps=a.reps, images_per_s=a.clouds / (np.median(times) / 1e3), tool_s=tool_s,
                    oracle_s_per_image=oracle_s, oracle_images=a.oracle_images,
                    oracle_s_split_scaled=oracle_s * a.clouds, device=torch.cuda.get_device_name(dev))
        BL.emit(line, a.out)


if __name__ == "__main__":
    main()
