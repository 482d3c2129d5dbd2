#!/usr/bin/env python3
"""Wall time of the ground-truth voxel downsampling at the chair test split's shape: dpc.render.downsample_split (batched,
end to end from host arrays to the per-model numpy results) against the numpy oracle of tests/test_downsample_host.py on a
few clouds, scaled to the split.  Prints one JSON line.

The split: data/splits/03001627_test.txt has 1 356 models.  The dense clouds are assumed to hold 120 000 points (float64,
as loadmat returns them): 100 000 edge midpoints (densify_single.py) plus the mesh vertices, whose count is not known here.
They are sampled on the faces of a few random boxes, a closed surface, so the reduction ratio is shape-like; the output
size recorded ("voxels_per_cloud") is what tools/bench_icp.py and tools/bench_chamfer.py assume as the GT size.

    python tools/bench_downsample.py [--models 1356] [--n-dense 120000] [--voxel 0.01] [--clouds-per-call 256]
                                     [--oracle-models 3] [--reps 2]

kernel_ms sums the library's per-launch events over one whole split; sort_pass_* is per kernel: the bytes one digit pass
must move (8 B key read by k_ds_hist; 12 B key + row read and written by k_ds_scatter, per member) over the time of the
passes' kernels, against the 8.0 TB/s HBM peak.  single_voxel_200k_ms is one call on a 200 000-point cloud that is one
voxel: k_ds_average's longest serial chain."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np
import torch

import dpc.render as R
from dpc.render import _native


def box_surface(n, rng, boxes=4):
    """n points on the faces of `boxes` random boxes inside [-0.5, 0.5]^3."""
    k = rng.multinomial(n, np.ones(boxes) / boxes)
    parts = []
    for m in k:
        lo = rng.uniform(-0.5, 0.2, 3)
        hi = lo + rng.uniform(0.05, 0.3, 3)
        area = np.array([(hi[1] - lo[1]) * (hi[2] - lo[2]), (hi[0] - lo[0]) * (hi[2] - lo[2]), (hi[0] - lo[0]) * (hi[1] - lo[1])])
        u = rng.uniform(lo, hi, size=(m, 3))
        axis = rng.choice(3, size=m, p=area / area.sum())
        u[np.arange(m), axis] = np.where(rng.integers(0, 2, m) == 1, hi[axis], lo[axis])
        parts.append(u)
    return np.concatenate(parts)


def key_bits(clouds, vs):
    """The digit passes the library plans for one call (include/dpc_render.h): cloud-index bits plus per-axis key bits."""
    kmax = np.zeros(3)
    for c in clouds:
        lo = c.min(0) - vs * 0.5
        kmax = np.maximum(kmax, np.floor((c.max(0) - lo) / vs))
    bits = int(len(clouds) - 1).bit_length() + sum(int(k).bit_length() for k in kmax)
    return bits, math.ceil(bits / 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=1356)
    ap.add_argument("--n-dense", type=int, default=120000)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--clouds-per-call", type=int, default=256)
    ap.add_argument("--oracle-models", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    clouds = [box_surface(a.n_dense, rng) for _ in range(a.models)]
    names = list(range(a.models))
    dev = torch.device("cuda")

    out = None

    def call():
        nonlocal out
        out = R.downsample_split(names, clouds.__getitem__, a.voxel, clouds_per_call=a.clouds_per_call)

    R.downsample_split(names[:8], clouds.__getitem__, a.voxel)            # warm-up: code objects, allocator
    walls = [ms / 1e3 for ms in BL.walls_ms(call, a.reps, warmup=0)]
    wall = min(walls)
    prof = _native.profile_kernels(call, dev)
    kern_ms = {k: round(sum(v), 3) for k, v in prof.items()}

    # per-kernel rate of the digit passes: the passes each call needs, their bytes over the three kernels' time
    moved = 0
    for g in range(0, a.models, a.clouds_per_call):
        group = clouds[g:g + a.clouds_per_call]
        moved += key_bits(group, a.voxel)[1] * 32.0 * sum(len(c) for c in group)
    sort_ms = sum(kern_ms.get(k, 0.0) for k in ("k_ds_hist", "k_ds_digits", "k_ds_scatter"))
    sizes = np.array([len(out[n]) for n in names])

    # the numpy oracle, scaled to the split
    from test_downsample_host import oracle_downsample

    no = min(a.oracle_models, a.models)
    t0 = time.perf_counter()
    for m in range(no):
        ref = oracle_downsample(clouds[m], a.voxel)
        assert ref.tobytes() == out[m].tobytes(), m
    oracle_s = (time.perf_counter() - t0) / no * a.models

    # the longest serial chain k_ds_average can get: one call on a single 200 000-point voxel
    one = rng.random((200000, 3)) * (a.voxel * 0.45)
    R.voxel_down_sample([one], a.voxel)
    prof1 = _native.profile_kernels(lambda: R.voxel_down_sample([one], a.voxel), dev)

    res = {
        "bench": "downsample_split", "models": a.models, "n_dense": a.n_dense, "dense_size_assumed": True,
        "voxel_size": a.voxel, "clouds_per_call": a.clouds_per_call, "dtype": "float64",
        "wall_s": round(wall, 4), "walls_s": [round(w, 4) for w in walls],
        "points_per_s": a.models * a.n_dense / wall,
        "kernel_ms_split": kern_ms, "kernel_ms_total": round(sum(kern_ms.values()), 3),
        "key_bits_first_call": key_bits(clouds[:a.clouds_per_call], a.voxel)[0],
        "sort_passes_first_call": key_bits(clouds[:a.clouds_per_call], a.voxel)[1],
        "sort_pass_bytes": moved, "sort_pass_kernel_ms": round(sort_ms, 3),
        "sort_pass_bytes_per_s": moved / (sort_ms * 1e-3), "sort_pass_share_of_hbm_peak": moved / (sort_ms * 1e-3) / BL.HBM_PEAK,
        "voxels_per_cloud": {"mean": float(sizes.mean()), "min": int(sizes.min()), "max": int(sizes.max())},
        "numpy_oracle_s_scaled": round(oracle_s, 2), "numpy_oracle_models_timed": no,
        "speedup_vs_numpy_oracle": round(oracle_s / wall, 1),
        "single_voxel_200k_ms": {k: round(sum(v), 3) for k, v in prof1.items() if k in ("k_ds_average", "k_ds_bounds")},
        "device": torch.cuda.get_device_name(0),
    }
    BL.emit(res)


if __name__ == "__main__":
    main()
