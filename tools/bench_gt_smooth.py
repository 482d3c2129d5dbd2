#!/usr/bin/env python3
"""Time of the ground-truth node (dpc.render.smooth_gt, csrc/dpc_gt_smooth.hip: resize + two-pass blur in one launch) against
the same rule composed on the device from F.avg_pool2d (or strided sampling) plus two F.conv2d, and of one full TrainStep with
and without cfg.pc_gauss_filter_gt.  Prints one JSON line per shape and appends it to profiles/gt_smooth_bench.jsonl (--out).

    python tools/bench_gt_smooth.py [--reps 200] [--warmup 20] [--windows 5] [--out FILE] [--no-step]
    python tools/bench_gt_smooth.py --route new|torch --reps 20 --no-step    (one route alone, for rocprofv3 --kernel-trace --stats)
    python tools/bench_gt_smooth.py --resource-usage [FILE]                  (no device: the compiler's registers and LDS)

Shapes: S = 32 masks of 128 x 128 to 64 x 64 (mean) at 11 and 21 taps, S = 32 images of 128 x 128 x 3 to 64 x 64 (sample) at 11
taps.  wall_ms: device events around `reps` back-to-back calls through dpc.render.smooth_gt (Python, ctypes and the launch
included), after `warmup` calls of every timed shape; the two routes alternate in windows, the median window is reported
with the spread.  kernel_ms: the library's own event pair around the launch (dpc_profile_enable), median of `reps` single
launches, with what an empty event pair reads on the same stream next to it; kernel times under rocprofv3 come from a run
with --route.  bytes: what the node must move (the source read once, the output written once), computed from the shapes;
the share of the HBM peak is bytes / kernel_ms over 8 TB/s.  The two routes' outputs are compared at the timed size before
anything is timed; more than 1e-5 apart ends the run.  The step: dpc.harness.config.chair_unsupervised with --step-batch
objects (64^3, 8000 points, 4 pose candidates, 128 x 128 masks, no point dropout), eager, with and without the key: a host
clock around `--step-reps` steps that end in a synchronise, the two configurations alternating in windows, medians."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL

SHAPES = (("masks", 32, 128, 64, 11, 1.5), ("masks", 32, 128, 64, 21, 3.0), ("images", 32, 128, 64, 11, 1.5))


def resource_usage(path):
    BL.resource_usage("dpc_gt_smooth.hip", path, [
        "# dynamic LDS on top of the static figure: (16 + 2c) x (128 + 2c) x 4 bytes for 2c + 1 taps: 14,352 B at 11 taps, "
        "21,312 B at 21, 59,280 B at 63"], keep="k_gt_smooth")


def composed(gt, C, f, mode_mean, w):
    """The same rule from torch's own device kernels: [S,C,Hs,Ws] -> [S,H,W,C]."""
    import torch.nn.functional as F

    n = w.numel()
    g = F.avg_pool2d(gt, f) if mode_mean else gt[:, :, ::f, ::f]
    g = F.conv2d(g, w.reshape(1, 1, 1, n).repeat(C, 1, 1, 1), padding=(0, n // 2), groups=C)
    g = F.conv2d(g, w.reshape(1, 1, n, 1).repeat(C, 1, 1, 1), padding=(n // 2, 0), groups=C)
    return g.permute(0, 2, 3, 1).contiguous()


def bench_shape(a, kind, S, src, dst, taps, sigma):
    import torch

    import dpc.render as R
    from dpc.harness.config import chair_unsupervised
    from dpc.render import _native

    dev = torch.device("cuda")
    C = 3 if kind == "images" else 1
    cfg = chair_unsupervised(vox_size=dst, pc_gauss_kernel_size=taps)
    gen = torch.Generator().manual_seed(27)
    gt = torch.rand(S, C, src, src, generator=gen)
    gt = ((gt < 0.45).float() if kind == "masks" else gt).to(dev)
    w = R.gauss_kernel_1d(taps, sigma).to(dev)

    def new():
        return R.smooth_gt(cfg, gt, dst, kind, sigma_rel=sigma)

    def old():
        return composed(gt, C, src // dst, kind == "masks", w)

    diff = float((new() - old()).abs().max())
    if diff > 1e-5:
        raise SystemExit("the two routes disagree at %s: %.3e" % ((kind, S, src, dst, taps), diff))
    fns = {"new": new, "torch": old}
    if a.route:
        fns = {a.route: fns[a.route]}
    med, spread = BL.event_windows(fns, a.reps, a.warmup, a.windows, digits=5)
    med = {k + "_wall_ms": v for k, v in med.items()}
    nbytes = 4 * S * C * (src * src + dst * dst)
    res = {"bench": "gt_smooth", "kind": kind, "samples": S, "channels": C, "source": src, "size": dst, "taps": taps,
           "reps": a.reps, "warmup": a.warmup, "windows": a.windows, "timing": "device events, median window", **med,
           "spread_ms": spread,
           "bytes_moved": nbytes, "max_abs_diff_of_routes": diff, "device": torch.cuda.get_device_name(0)}
    if "new" in fns:
        rec = _native.profile_kernels(lambda: [new() for _ in range(a.reps)], dev).get("k_gt_smooth", [])
        if rec:
            k_ms = BL.upper_median(rec)
            res.update(new_kernel_ms=round(k_ms, 5), new_kernel_launches_per_call=len(rec) / a.reps,
                       empty_event_pair_ms=round(_native.event_pair_overhead_ms(dev), 5),
                       kernel_timing="the library's event pair around the launch, median; includes what an empty pair reads",
                       new_fraction_of_hbm_peak=BL.share(nbytes, k_ms, BL.HBM_PEAK, 4))
    if "new_wall_ms" in med and "torch_wall_ms" in med:
        res["speedup_wall"] = round(med["torch_wall_ms"] / med["new_wall_ms"], 2)
    BL.emit(res, a.out)


def bench_step(a):
    """One full eager TrainStep (the experiments' configuration: 64^3, 8000 points, K = 4, batch_size x step_size views) with and
    without cfg.pc_gauss_filter_gt, alternating; host clock around a synchronised step."""
    import torch

    from dpc.harness import TrainStep
    from dpc.harness.config import chair_unsupervised

    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(3)
    steps = {}
    for key in (False, True):
        cfg = chair_unsupervised(batch_size=a.step_batch, pc_point_dropout=1.0, pc_gauss_filter_gt=key)
        torch.manual_seed(0)
        steps[key] = (cfg, TrainStep(cfg, dev))
    cfg = steps[False][0]
    views = cfg.batch_size * cfg.step_size
    side = cfg.input_shape[0]
    images = torch.rand(views, 3, side, side, generator=gen).to(dev)
    masks = (torch.rand(views, 1, side, side, generator=gen) < 0.45).float().to(dev)

    def run(key, n):
        return BL.batch_ms(lambda: steps[key][1](images, masks), n, warmup=0)

    for key in steps:
        run(key, a.step_warmup)
    times = {False: [], True: []}
    for _ in range(a.windows):
        for key in steps:
            times[key].append(run(key, a.step_reps))
    med = {k: BL.upper_median(v) for k, v in times.items()}
    res = {"bench": "gt_smooth_step", "views": views, "grid": cfg.vox_size, "points": cfg.pc_num_points,
           "candidates": cfg.pose_predict_num_candidates, "mask_side": side, "taps": cfg.pc_gauss_kernel_size,
           "reps": a.step_reps, "warmup": a.step_warmup, "windows": a.windows,
           "timing": "host clock around synchronised eager steps, median window",
           "step_ms_without_key": round(med[False], 4), "step_ms_with_key": round(med[True], 4),
           "spread_ms": {"without": [round(min(times[False]), 4), round(max(times[False]), 4)],
                         "with": [round(min(times[True]), 4), round(max(times[True]), 4)]},
           "added_ms": round(med[True] - med[False], 4), "device": torch.cuda.get_device_name(0)}
    BL.emit(res, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--route", choices=("new", "torch"), default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "gt_smooth_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "gt_smooth_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_gt_smooth.py times kernels on an MI355X: no HIP device here")
    for shape in SHAPES:
        bench_shape(a, *shape)
    if not a.no_step:
        bench_step(a)


if __name__ == "__main__":
    main()
