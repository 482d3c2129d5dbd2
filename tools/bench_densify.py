#!/usr/bin/env python3
"""Wall time of the ground-truth mesh densification: dpc.render.densify_split (batched, end to end from host meshes to
the per-model numpy results) on synthetic meshes, against the heap oracle of tests/densify_oracle.py on one mesh.  Prints
one JSON line.

The meshes: a UV sphere plus an axis-aligned box (tests/densify_oracle.sphere_box_obj), 6 228 faces by default, each
model's sphere moved a little so no two are equal.  Real ShapeNet face counts were not measured here: --lat/--lon/--box-div
set the assumed size, and the JSON line states the face count used.

    python tools/bench_densify.py [--models 256] [--num-points 100000] [--models-per-call 256] [--lat 40] [--lon 76]
                                  [--box-div 5] [--reps 2] [--reference-s 57]

kernel_ms sums the library's per-launch events over one whole job.  rounds is the number of rounds the batch needed (the
most any model needed), found by a run that reads the counter after every round.  oracle_s_per_model times the
host oracle (a heap restatement of the reference) on one mesh.  reference_cpu_s_per_model is not measured by this tool:
it is the reference's own densify_model time for a 6 252-face mesh, passed in with --reference-s."""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np
import torch

import densify_oracle as D
import dpc.render as R
from dpc.render import _native
from dpc.render import densify as RD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--num-points", type=int, default=100000)
    ap.add_argument("--models-per-call", type=int, default=256)
    ap.add_argument("--lat", type=int, default=40)
    ap.add_argument("--lon", type=int, default=76)
    ap.add_argument("--box-div", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--reference-s", type=float, default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    meshes = []
    with tempfile.TemporaryDirectory() as tmp:
        for m in range(a.models):
            path = os.path.join(tmp, "m.obj")
            with open(path, "w") as fh:
                fh.write(D.sphere_box_obj(a.lat, a.lon, box_div=a.box_div, center=tuple(rng.uniform(-0.05, 0.05, 3))))
            meshes.append(R.load_obj_mesh(path))
    faces = int(np.mean([len(m[2]) for m in meshes]))
    names = list(range(a.models))
    dev = torch.device("cuda")
    out = None

    def call():
        nonlocal out
        out = R.densify_split(names, meshes.__getitem__, a.num_points, models_per_call=a.models_per_call)

    R.densify_split(names[:2], meshes.__getitem__, 1000)  # warm-up: code objects, allocator
    walls = [ms / 1e3 for ms in BL.walls_ms(call, a.reps, warmup=0)]
    wall = min(walls)
    prof = _native.profile_kernels(call, dev, capacity=65536)
    kern_ms = {k: round(sum(v), 3) for k, v in prof.items()}
    launches = {k: len(v) for k, v in prof.items()}
    # the rounds the first job needs: counter read after every round
    group = [RD._mesh(m, i) for i, m in enumerate(meshes[:a.models_per_call])]
    _, _, rounds = RD._densify_packed(group, a.num_points, rounds_per_sync=1)

    t0 = time.perf_counter()
    ref = D.oracle_densify(*meshes[0], a.num_points)
    oracle_s = time.perf_counter() - t0
    assert ref.tobytes() == out[0].tobytes(), "the GPU result differs from the oracle"

    res = {
        "bench": "densify_split", "models": a.models, "num_points": a.num_points, "models_per_call": a.models_per_call,
        "faces_per_model": faces, "faces_assumed_synthetic": True, "vertices_per_model": int(len(meshes[0][0])),
        "wall_s": round(wall, 4), "walls_s": [round(w, 4) for w in walls],
        "wall_s_per_model": wall / a.models,
        "kernel_ms_job": kern_ms, "kernel_ms_total": round(sum(kern_ms.values()), 3), "launches": launches,
        "rounds_first_job": rounds,
        "oracle_s_per_model": round(oracle_s, 2),
        "reference_cpu_s_per_model": a.reference_s,
        "speedup_vs_oracle": round(oracle_s * a.models / wall, 1),
        "device": torch.cuda.get_device_name(0),
    }
    if a.reference_s:
        res["speedup_vs_reference"] = round(a.reference_s * a.models / wall, 1)
    BL.emit(res)


if __name__ == "__main__":
    main()
