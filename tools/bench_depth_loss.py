#!/usr/bin/env python3
"""Time of the expected-depth loss (dpc.render.proj_depth_loss: forward, and forward + backward) against the route the
package had before it: the lazy outputs["proj_depth"] entry (D-pass launch, scale and clamp in torch, Drc with its [D+1,B,H,W]
probabilities, flip, multiply by psi, sum) followed by the same loss in torch, differentiated by autograd.  Prints one JSON
line per run and appends it to profiles/depth_loss_bench.jsonl (--out).

The shape: B = 32 clouds of 8 000 points, 64^3 grid, 21-tap Gaussian at sigma_rel 0.64, depth maps at twice the projection's
size (f = 2), learned occupancy scale.  Both routes start from the SAME fused projection (pointcloud_project_fast runs once,
outside the timed region); what is timed is the depth loss on top of it, down to the gradients at grid_wh and s -- where
the fused node's own backward takes over in either route.  `step_*`: the whole of projection + silhouette loss + depth loss +
backward, for scale.

    python tools/bench_depth_loss.py [--clouds 32] [--points 8000] [--grid 64] [--reps 200] [--warmup 50] [--route both]
                                     [--out FILE]

GPU time by device events around `reps` back-to-back calls after `warmup` calls of the same shape; the two routes alternate
in windows.  --route new|lazy with --reps small: one route alone, for a run under rocprofv3 --kernel-trace --stats."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import torch

import dpc.render as R


class Cfg(dict):
    __getattr__ = dict.__getitem__


def torch_loss(cfg, pred, depths, f):
    """The loss of proj_depth_loss written on outputs["proj_depth"] with torch, as a caller had to before."""
    g = depths[:, ::f, ::f, :]
    if cfg.max_depth != cfg.max_dataset_depth:
        g = torch.where(g == cfg.max_dataset_depth, torch.full_like(g, cfg.max_depth), g)
    return 0.5 * ((g - pred) ** 2).sum() / pred.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--route", default="both", choices=["both", "new", "lazy"])
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "depth_loss_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, N, G, f = a.clouds, a.points, a.grid, 2
    cfg = Cfg(vox_size=G, vox_size_z=-1, pc_gauss_kernel_size=21, camera_distance=2.0, focal_length=1.875,
              drc_logsum_clip_val=1e-5, max_depth=10.0, max_dataset_depth=10.0)
    gen = torch.Generator().manual_seed(1234)
    pc = (torch.tanh(0.5 * torch.randn(B, N, 3, generator=gen)) / 2).float().to(dev).requires_grad_(True)
    q = torch.randn(B, 4, generator=gen).float().to(dev).requires_grad_(True)
    s = (0.5 + 0.5 * torch.rand(B, 1, generator=gen)).float().to(dev).requires_grad_(True)
    masks = (torch.rand(B, 1, f * G, f * G, generator=gen) > 0.5).float().to(dev)
    depths = (1.5 + 1.5 * torch.rand(B, f * G, f * G, 1, generator=gen)).float()
    depths[torch.rand(B, f * G, f * G, 1, generator=gen) < 0.3] = cfg.max_dataset_depth
    depths = depths.to(dev)
    kernel = R.smoothing_kernel(cfg, 0.64)

    # one projection; the depth loss of both routes starts at its grid_wh and s, as leaves
    with torch.no_grad():
        base = R.pointcloud_project_fast(cfg, pc, q, None, None, kernel, scaling_factor=s)
    geom, grid_wh, _ = base._fused
    grid = grid_wh.detach().clone().requires_grad_(True)
    sl = s.detach().clone().requires_grad_(True)

    def outputs_new():
        return R.ProjectionOutputs(base["proj"], {}, fused=(geom, grid, sl))

    def outputs_lazy():
        return R.ProjectionOutputs(base["proj"], R._outputs_from_grid(cfg, geom, grid, pc, q, None, None, sl, None))

    def new_fwd():
        with torch.no_grad():
            return R.proj_depth_loss(cfg, outputs_new(), depths)

    def lazy_fwd():
        with torch.no_grad():
            return torch_loss(cfg, outputs_lazy()["proj_depth"], depths, f)

    def new_both():
        grid.grad = sl.grad = None
        R.proj_depth_loss(cfg, outputs_new(), depths).backward()

    def lazy_both():
        grid.grad = sl.grad = None
        torch_loss(cfg, outputs_lazy()["proj_depth"], depths, f).backward()

    def step(route):
        def run():
            pc.grad = q.grad = s.grad = None
            out = R.pointcloud_project_fast(cfg, pc, q, None, None, kernel, scaling_factor=s)
            sil, _ = R.silhouette_loss(out["proj"], masks)
            dl = R.proj_depth_loss(cfg, out, depths) if route == "new" else torch_loss(cfg, out["proj_depth"], depths, f)
            (sil + 0.5 * dl).backward()
        return run

    fns = {"new_forward_ms": new_fwd, "lazy_forward_ms": lazy_fwd, "new_forward_backward_ms": new_both,
           "lazy_forward_backward_ms": lazy_both, "step_new_ms": step("new"), "step_lazy_ms": step("lazy")}
    if a.route != "both":
        fns = {k: v for k, v in fns.items() if a.route in k}
    # the two routes compute the same thing
    agree = None
    if a.route == "both":
        new_both()
        g_new, s_new, l_new = grid.grad.clone(), sl.grad.clone(), float(new_fwd())
        lazy_both()
        scale = max(1.0, float(grid.grad.abs().max()))
        # the lazy route's D pass keeps all 21 taps, the column kernels the 7 that matter in fp32: voxels whose s v sits within
        # ~1e-9 of the clamp at eps are decided differently, and such a voxel's gradient is there in one route and 0 in the
        # other (tests/test_gpu_parity.py::test_drc_clamp_threshold_flip_is_bounded_and_explained); counted here
        diff = (g_new - grid.grad).abs()
        agree = {"loss_rel_diff": abs(l_new - float(lazy_fwd())) / abs(l_new),
                 "dgrid_max_abs_diff_over_scale": float(diff.max()) / scale,
                 "dgrid_voxels": diff.numel(), "dgrid_voxels_off_by_1e-5_scale": int((diff > 1e-5 * scale).sum()),
                 "dgrid_columns_off": int((diff > 1e-5 * scale).any(dim=1).sum()),
                 "ds_max_rel_diff": float(((s_new - sl.grad).abs() / sl.grad.abs().clamp_min(1.0)).max())}
    med, spread = BL.event_windows(fns, a.reps, a.warmup, a.windows)
    grid_mb = B * G * G * G * 4 / 1e6
    res = {"bench": "depth_loss", "clouds": B, "points": N, "grid": G, "gt_factor": f, "sigma_rel": 0.64, "taps": 21,
           "reps": a.reps, "warmup": a.warmup, "windows": a.windows, "route": a.route, "timing": "device events, median window",
           "grid_mb": round(grid_mb, 1), **med,
           "spread_ms": spread,
           "device": torch.cuda.get_device_name(0)}
    if a.route == "both":
        res["speedup_forward"] = round(med["lazy_forward_ms"] / med["new_forward_ms"], 2)
        res["speedup_forward_backward"] = round(med["lazy_forward_backward_ms"] / med["new_forward_backward_ms"], 2)
        res["speedup_step"] = round(med["step_lazy_ms"] / med["step_new_ms"], 3)
        res["agreement"] = agree
    BL.emit(res, a.out)


if __name__ == "__main__":
    main()
