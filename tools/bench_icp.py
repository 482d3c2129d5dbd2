#!/usr/bin/env python3
"""Throughput of the batched ICP (dpc.render.icp_point_to_point) at compute_alignment's size, with a 16-thread
scipy.spatial.cKDTree ICP of the same semantics on the CPU as the baseline.  Prints one JSON line.

The batch: 50 models x 5 views = 250 pairs, n_src = 8000 predicted points per view, GT clouds of 16 384 points shared by
the 5 views of a model, camera errors (ICP init) up to 30 degrees.  The real size of the downsampled ShapeNet GT clouds
is not known here: the GT size is an assumption, and the cost scales linearly with it.

    python tools/bench_icp.py [--models 50] [--views 5] [--n-src 8000] [--n-tgt 16384] [--cpu-pairs 10] [--reps 3]

The CPU baseline runs --cpu-pairs pairs (cKDTree query with workers=16, Umeyama by SVD, same stopping rule) and is
scaled to the whole batch."""
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


def rot(axis, angle):
    axis = np.asarray(axis) / np.linalg.norm(axis)
    return R.as_rotation_matrix(np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])[None])[0]


def cpu_icp(src, tgt, tau, init, max_iteration=30, rel=1e-6):
    from scipy.spatial import cKDTree

    tree = cKDTree(tgt)
    T = init.copy()
    cur = src @ T[:3, :3].T + T[:3, 3]

    def evaluate(cur):
        d, j = tree.query(cur, k=1, distance_upper_bound=tau, workers=16)
        inl = d < tau
        n = int(inl.sum())
        if n == 0:
            return 0.0, 0.0, None, None
        return n / len(cur), float(np.sqrt((d[inl] ** 2).sum() / n)), cur[inl], tgt[j[inl]]

    fit, rmse, p, q = evaluate(cur)
    it = 0
    for it in range(1, max_iteration + 1):
        upd = np.eye(4)
        if p is not None:
            mp, mq = p.mean(0), q.mean(0)
            U, _, Vt = np.linalg.svd((q - mq).T @ (p - mp) / len(p))
            D = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
            upd[:3, :3] = U @ D @ Vt
            upd[:3, 3] = mq - upd[:3, :3] @ mp
        T = upd @ T
        cur = cur @ upd[:3, :3].T + upd[:3, 3]
        f0, r0 = fit, rmse
        fit, rmse, p, q = evaluate(cur)
        if abs(f0 - fit) < rel and abs(r0 - rmse) < rel:
            break
    return T, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=50)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--n-src", type=int, default=8000)
    ap.add_argument("--n-tgt", type=int, default=16384)
    ap.add_argument("--cpu-pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    targets, sources, target_of, inits = [], [], [], []
    for m in range(a.models):
        gt = shape_cloud(a.n_tgt, rng) * rng.uniform(0.8, 1.2, size=3)
        targets.append(gt)
        for v in range(a.views):
            sources.append((gt[rng.permutation(a.n_tgt)[:a.n_src]] + rng.normal(size=(a.n_src, 3)) * 0.005).astype(np.float32))
            init = np.eye(4)
            init[:3, :3] = rot(rng.normal(size=3), rng.uniform(0, np.pi / 6))   # init error up to 30 degrees
            inits.append(init)
            target_of.append(m)
    P = len(sources)
    inits = np.stack(inits)
    call = lambda: R.icp_point_to_point(sources, targets, 0.2, init=inits, target_of=target_of)
    out = call()
    walls = [ms / 1e3 for ms in BL.walls_ms(call, a.reps, warmup=0)]
    wall = BL.upper_median(walls)
    iters = out[3].cpu().numpy()
    rounds = iters.astype(np.float64) + 1   # evaluations per pair
    pair_evals = float((rounds * a.n_src * a.n_tgt).sum())
    prof = _native.profile_kernels(call, dev)
    kern_ms = {k: round(sum(v) / 1.0, 3) for k, v in prof.items()}

    torch.set_num_threads(16)
    idx = np.linspace(0, P - 1, min(a.cpu_pairs, P)).astype(int)
    t0 = time.perf_counter()
    cpu_iters = []
    for i in idx:
        _, it = cpu_icp(sources[i].astype(np.float64), targets[target_of[i]], 0.2, inits[i])
        cpu_iters.append(it)
    cpu_per_pair = (time.perf_counter() - t0) / len(idx)
    cpu_total = cpu_per_pair * P
    hist = np.bincount(iters, minlength=31).tolist()
    BL.emit({
        "bench": "icp_point_to_point", "pairs": P, "n_src": a.n_src, "n_tgt": a.n_tgt, "gt_size_assumed": True,
        "wall_s": round(wall, 4), "walls_s": [round(w, 4) for w in walls],
        "pair_evals": pair_evals, "pair_evals_per_s": pair_evals / wall,
        "iterations_hist": hist, "mean_iterations": float(iters.mean()),
        "kernel_ms_one_call": kern_ms,
        "cpu_ckdtree16_s_per_pair": round(cpu_per_pair, 4), "cpu_ckdtree16_s_scaled": round(cpu_total, 2),
        "cpu_pairs_timed": len(idx), "cpu_iterations": cpu_iters, "speedup_vs_cpu": round(cpu_total / wall, 1),
        "device": torch.cuda.get_device_name(0),
    })


if __name__ == "__main__":
    main()
