#!/usr/bin/env python3
"""Time of farthest-point sampling (dpc.render.farthest_point_sample) at the evaluation's shapes: 256 fp32 clouds of 8000
points to 1024 and to 2048 samples (the predictions), and 256 fp64 clouds of 12647 points to 1024 samples (the largest
voxel-downsampled ground-truth cloud).  Per shape: wall time of the call, kernel time from the library's launch record,
and time per round; and two baselines measured in the same run:

    torch loop   the same rule composed from torch ops on the device, one batched loop of m rounds (what a user would
                 write without the kernel); its indices are compared with the kernel's
    numpy        the oracle of tests/fps_oracle.py on the host for --host-clouds clouds, scaled to the batch

--split adds the time of emd_of_split with sampling="fps" against "random" (--models models of --views views of 8000
points against ground-truth clouds of 12647 points, 1024 samples).  Prints one JSON line per shape and appends them to
profiles/fps_bench.jsonl (--out).

    python tools/bench_fps.py [--clouds 256] [--reps 5] [--torch-reps 2] [--host-clouds 2] [--split] [--out FILE]
    python tools/bench_fps.py --resource-usage [FILE]     (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after two warm-up calls, each call ended by a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np

SHAPES = [(8000, "float32", 1024), (8000, "float32", 2048), (12647, "float64", 1024)]


def resource_usage(path):
    BL.resource_usage("dpc_fps.hip", path, [
        "# k_fps<fp64 input, threads, points per thread>; lds= is the static part (what __syncthreads_or reserves), the",
        "# dynamic part is 12 bytes per wave + 32, and for k_fps<1, 1024, 16> also dist, 8 bytes per point: 131296 B"])


def torch_loop(pts, m):
    """The rule of dpc_fps from torch ops, batched over [B,n,3] (fp64 arithmetic): [B,m] int64 indices."""
    import torch

    P = pts.double()
    B, n, _ = P.shape
    rows = torch.arange(B, device=P.device)
    dist = torch.full((B, n), float("inf"), dtype=torch.float64, device=P.device)
    taken = torch.zeros((B, n), dtype=torch.bool, device=P.device)
    cur = torch.zeros((B,), dtype=torch.int64, device=P.device)
    out = torch.empty((B, m), dtype=torch.int64, device=P.device)
    for k in range(m):
        out[:, k] = cur
        taken[rows, cur] = True
        d = P - P[rows, cur][:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        dist = torch.minimum(dist, d2)
        cur = torch.where(taken, -1.0, dist).argmax(dim=1)
    return out


def bench_split(a, R, torch):
    rng = np.random.default_rng(5)
    preds = [((rng.random((a.views, 8000, 3)) - 0.5).astype(np.float32), None) for _ in range(a.models)]
    gts = [rng.random((12647, 3)) - 0.5 for _ in range(a.models)]
    res = {"bench": "emd_of_split_sampling", "models": a.models, "views": a.views, "pred_points": 8000, "gt_points": 12647,
           "num_points": 1024, "reps": a.split_reps, "device": torch.cuda.get_device_name(0)}
    for mode in ("random", "fps"):
        t = BL.median_ms(lambda: R.emd_of_split(preds, gts, num_points=1024, seed=0, sampling=mode), a.split_reps, warmup=1, digits=None)
        res["%s_ms" % mode] = round(t[0], 2)
        res["%s_ms_min_max" % mode] = [round(t[1], 2), round(t[2], 2)]
        res["%s_mean_emd" % mode] = float(R.emd_of_split(preds, gts, num_points=1024, seed=0, sampling=mode).mean())
    res["fps_over_random"] = round(res["fps_ms"] / res["random_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--host-clouds", type=int, default=2)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--models", type=int, default=32)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--split-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "fps_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "fps_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    import dpc.render as R
    import fps_oracle
    from dpc.render import _native

    dev = torch.device("cuda")
    lines = []
    for n, dtype, m in SHAPES:
        B = a.clouds
        rng = np.random.default_rng(1000 * n + m)
        host = (rng.random((B, n, 3)) - 0.5).astype(dtype)
        pts = torch.from_numpy(host).to(dev)
        wall = BL.median_ms(lambda: R.farthest_point_sample(pts, m), a.reps, warmup=2, digits=None)
        prof = _native.profile_kernels(lambda: R.farthest_point_sample(pts, m), dev)
        kernel_ms = float(sum(sum(v) for k, v in prof.items() if k.startswith("k_fps")))
        ids = sorted(i for i in _native.launched_instantiations(lambda: R.farthest_point_sample(pts, m), dev) if i.startswith("k_fps"))
        idx = R.farthest_point_sample(pts, m)
        assert R.check_status() == 0
        loop = BL.median_ms(lambda: torch_loop(pts, m), a.torch_reps, warmup=1, digits=None)
        agree = float((torch_loop(pts, m) == idx.long()).all(dim=1).double().mean())
        k = min(a.host_clouds, B)
        host_ms = []
        for c in range(k):
            t0 = time.perf_counter()
            ref = fps_oracle.fps(host[c], m)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert ref[0].tolist() == idx[c].cpu().tolist()
        res = {
            "bench": "fps", "clouds": B, "n": n, "dtype": dtype, "samples": m, "reps": a.reps, "kernels": ids,
            "wall_ms": round(wall[0], 3), "wall_ms_min_max": [round(wall[1], 3), round(wall[2], 3)],
            "kernel_ms": round(kernel_ms, 3), "us_per_round": round(1e3 * kernel_ms / m, 3),
            "torch_loop_ms": round(loop[0], 2), "torch_loop_ms_min_max": [round(loop[1], 2), round(loop[2], 2)],
            "torch_loop_us_per_round": round(1e3 * loop[0] / m, 2), "torch_loop_clouds_with_equal_indices": agree,
            "speedup_vs_torch_loop": round(loop[0] / wall[0], 1),
            "numpy_clouds_timed": k, "numpy_host_ms_per_cloud": round(float(np.median(host_ms)), 1) if k else None,
            "numpy_host_ms_scaled_to_batch": round(float(np.median(host_ms)) * B, 1) if k else None,
            "device": torch.cuda.get_device_name(0),
        }
        lines.append(res)
    if a.split:
        lines.append(bench_split(a, R, torch))
    for res in lines:
        BL.emit(res, a.out)


if __name__ == "__main__":
    main()
