#!/usr/bin/env python3
"""Wall time of the Chamfer half of the evaluation at the chair test split's shape: dpc.render.chamfer_of_split (batched,
end to end from host arrays to the [M,V,2] array) against the per-view loop chamfer_of_predictions, and optionally a
16-worker scipy.spatial.cKDTree baseline.  Prints one JSON line.

The split: data/splits/03001627_test.txt has 1 356 models, 5 views each, 8 000 predicted points per view (float32, as
predict_to.py writes them).  The GT clouds are assumed to hold 16 384 points (float64, as loadmat returns them): their real
size is not known here (the same assumption as tools/bench_icp.py), and the cost scales linearly with it.

    python tools/bench_chamfer.py [--models 1356] [--views 5] [--n-pred 8000] [--n-gt 16384] [--loop-models 20]
                                  [--ckdtree-models 4] [--reps 2]

The per-view loop and the cKDTree baseline run on --loop-models / --ckdtree-models models (the first ones of the split)
and are scaled to the split; max_abs_diff compares path (a) with (b) on the models both computed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np
import torch

import dpc.render as R
from dpc.render import _native


def shape_cloud(n, rng):
    k = rng.multinomial(n, [0.5, 0.3, 0.2])
    slab = rng.uniform([-0.5, -0.3, -0.05], [0.5, 0.3, 0.05], size=(k[0], 3))
    rod = rng.uniform([0.3, 0.2, 0.0], [0.4, 0.3, 0.6], size=(k[1], 3))
    ball = rng.normal(size=(k[2], 3)) * 0.08 + [-0.35, -0.1, 0.25]
    return np.concatenate([slab, rod, ball])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=1356)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--n-pred", type=int, default=8000)
    ap.add_argument("--n-gt", type=int, default=16384)
    ap.add_argument("--loop-models", type=int, default=20)
    ap.add_argument("--ckdtree-models", type=int, default=4)
    ap.add_argument("--models-per-call", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    preds, gts = [], []
    for m in range(a.models):
        gt = shape_cloud(a.n_gt, rng) * rng.uniform(0.8, 1.2, size=3)
        gts.append(gt)
        pts = np.stack([shape_cloud(a.n_pred, rng) * rng.uniform(0.8, 1.2, size=3) for _ in range(a.views)]).astype(np.float32)
        preds.append((pts, None))
    dev = torch.device("cuda")
    pair_evals = 2.0 * a.models * a.views * a.n_pred * a.n_gt

    # (a) batched, end to end
    call = lambda: R.chamfer_of_split(preds, gts, models_per_call=a.models_per_call)
    out = call()
    walls = [ms / 1e3 for ms in BL.walls_ms(call, a.reps, warmup=0)]
    wall = min(walls)
    prof = _native.profile_kernels(call, dev)
    kern_ms = {k: round(sum(v), 3) for k, v in prof.items()}

    # (b) the per-view loop on the first --loop-models models, scaled to the split
    nl = min(a.loop_models, a.models)
    R.chamfer_of_predictions(preds[0][0], gts[0])      # warm-up
    old = []
    loop = lambda: old.extend(R.chamfer_of_predictions(preds[m][0], gts[m]) for m in range(nl))
    loop_s = BL.walls_ms(loop, 1, warmup=0)[0] / 1e3 / nl * a.models
    old = np.stack(old)
    diff = float(np.abs(old - out[:nl]).max())

    res = {
        "bench": "chamfer_of_split", "models": a.models, "views": a.views, "n_pred": a.n_pred, "n_gt": a.n_gt,
        "gt_size_assumed": True, "models_per_call": a.models_per_call,
        "wall_s": round(wall, 4), "walls_s": [round(w, 4) for w in walls],
        "pair_evals": pair_evals, "pair_evals_per_s": pair_evals / wall,
        "kernel_ms_one_call": kern_ms,
        "per_view_loop_s_scaled": round(loop_s, 3), "per_view_loop_models_timed": nl,
        "speedup_vs_per_view_loop": round(loop_s / wall, 2), "max_abs_diff_vs_per_view_loop": diff,
    }
    # (c) optional: scipy cKDTree with 16 workers, float64, scaled
    if a.ckdtree_models > 0:
        from scipy.spatial import cKDTree

        nk = min(a.ckdtree_models, a.models)
        t0 = time.perf_counter()
        for m in range(nk):
            gt = gts[m]
            tg = cKDTree(gt)
            for v in range(a.views):
                p = preds[m][0][v].astype(np.float64)
                tg.query(p, k=1, workers=16)[0].mean()
                cKDTree(p).query(gt, k=1, workers=16)[0].mean()
        res["cpu_ckdtree16_s_scaled"] = round((time.perf_counter() - t0) / nk * a.models, 3)
        res["cpu_ckdtree16_models_timed"] = nk
    res["device"] = torch.cuda.get_device_name(0)
    BL.emit(res)


if __name__ == "__main__":
    main()
