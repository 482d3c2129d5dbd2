#!/usr/bin/env python3
"""Time of the two ray-consistency losses (dpc.render.drc_loss and drc_rgb_loss: forward, and forward + backward) against the
composed route they replace: torch on the lazy outputs["drc_probs"] entry (D-pass launch, scale and clamp in torch, Drc with
its [D+1,B,H,W] probabilities, flip) and, for colour, on project_rgb(...)["voxels_rgb"], differentiated by autograd.  Prints one
JSON line per run and appends it to profiles/drc_loss_bench.jsonl (--out).

Shapes: mask loss B = 32 clouds, 64^3 grid, 21-tap Gaussian at sigma_rel 0.64, masks at twice the projection's size (f = 2),
learned occupancy scale; colour loss B = 32 clouds of 8 000 points, 64^3, 11 taps, images at twice the size.  Both routes
start from the SAME projection and the same colour grids (made once, outside the timed region); what is timed is the loss
on top of them, down to the gradients at (grid_wh, s) and (voxels, colour grid) -- where the renderer's own backward takes
over in either route.  The composed colour route calls project_rgb with the shared grids, so it also pays that function's
proj_rgb launch: it is what a caller gets voxels_rgb from.

    python tools/bench_drc_loss.py [--clouds 32] [--points 8000] [--grid 64] [--reps 100] [--warmup 20] [--route both]
                                   [--out FILE]

GPU time by device events around `reps` back-to-back calls after `warmup` calls of the same shape; the two routes alternate
in windows.  --route new|composed with --reps small: one route alone, for a run under rocprofv3 --kernel-trace --stats.
Bytes a kernel must move are computed from the shapes and printed next to the times."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import torch

import dpc.render as R


class Cfg(dict):
    __getattr__ = dict.__getitem__


def torch_mask_loss(probs, masks, f):
    """drc_loss written on outputs["drc_probs"] [D+1,B,H,W,1] with torch, as a caller had to before."""
    g = masks[:, 0, ::f, ::f]
    p = probs[..., 0]
    return ((1.0 - g) * p[:-1].sum(0) + g * p[-1]).sum() / masks.shape[0]


def torch_rgb_loss(probs, voxels_rgb, images, f):
    """drc_rgb_loss written on outputs["drc_probs"] [D+1,B,H,W,1] and voxels_rgb [B,D,H,W,3] with torch."""
    g = images[:, ::f, ::f]
    psi = ((g.unsqueeze(1) - voxels_rgb) ** 2).sum(-1)                  # [B,D,H,W]
    p = probs[..., 0]
    return ((p[:-1].permute(1, 0, 2, 3) * psi).sum() + (p[-1] * ((g - 1.0) ** 2).sum(-1)).sum()) / images.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--route", default="both", choices=["both", "new", "composed"])
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "drc_loss_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, N, G, f = a.clouds, a.points, a.grid, 2
    base_cfg = dict(vox_size=G, vox_size_z=-1, camera_distance=2.0, focal_length=1.875, drc_logsum_clip_val=1e-5, max_depth=10.0,
                    max_dataset_depth=10.0, pc_rgb_divide_by_occupancies=True, pc_rgb_divide_by_occupancies_epsilon=0.01)
    cfg_m, cfg_c = Cfg(pc_gauss_kernel_size=21, **base_cfg), Cfg(pc_gauss_kernel_size=11, **base_cfg)
    gen = torch.Generator().manual_seed(1234)
    pc = (torch.tanh(0.5 * torch.randn(B, N, 3, generator=gen)) / 2).float().to(dev)
    q = torch.randn(B, 4, generator=gen).float().to(dev)
    s = (0.5 + 0.5 * torch.rand(B, 1, generator=gen)).float().to(dev)
    rgb = torch.rand(B, N, 3, generator=gen).float().to(dev)
    masks = (torch.rand(B, 1, f * G, f * G, generator=gen) > 0.5).float().to(dev)
    images = torch.rand(B, f * G, f * G, 3, generator=gen).float().to(dev)
    kern_m, kern_c = R.smoothing_kernel(cfg_m, 0.64), R.smoothing_kernel(cfg_c, 0.64)

    # ---- mask loss: one projection; both routes start at its grid_wh and s, as leaves
    with torch.no_grad():
        base = R.pointcloud_project_fast(cfg_m, pc, q, None, None, kern_m, scaling_factor=s)
    geom, grid_wh, _ = base._fused
    grid = grid_wh.detach().clone().requires_grad_(True)
    sl = s.detach().clone().requires_grad_(True)

    def outputs_new():
        return R.ProjectionOutputs(base["proj"], {}, fused=(geom, grid, sl))

    def outputs_lazy():
        return R.ProjectionOutputs(base["proj"], R._outputs_from_grid(cfg_m, geom, grid, pc, q, None, None, sl, None))

    def mask_new_fwd():
        with torch.no_grad():
            return R.drc_loss(cfg_m, outputs_new(), masks)

    def mask_composed_fwd():
        with torch.no_grad():
            return torch_mask_loss(outputs_lazy()["drc_probs"], masks, f)

    def mask_new_both():
        grid.grad = sl.grad = None
        R.drc_loss(cfg_m, outputs_new(), masks).backward()

    def mask_composed_both():
        grid.grad = sl.grad = None
        torch_mask_loss(outputs_lazy()["drc_probs"], masks, f).backward()

    # ---- colour loss: one projection and one set of colour grids; both routes start at (voxels, colour grid), as leaves
    with torch.no_grad():
        cbase = R.pointcloud_project_fast(cfg_c, pc, q, None, None, kern_c, scaling_factor=s)
        cgeom, vox0, C0, div = R.rgb_grids(cfg_c, cbase, rgb, kern_c)
    vox = vox0.detach().clone().requires_grad_(True)
    C = C0.detach().clone().requires_grad_(True)
    grids = (cgeom, vox, C, div)

    def rgb_outputs():
        return R.ProjectionOutputs(cbase["proj"], lambda: {"voxels": vox.unsqueeze(-1), "tr_pc": None})

    def composed_rgb_loss():
        probs = R.drc_event_probabilities(vox.unsqueeze(-1), cfg_c)      # [D+1,B,H,W,1], grid order
        vrgb = R.project_rgb(cfg_c, rgb_outputs(), rgb, kern_c, grids=grids)["voxels_rgb"]
        return torch_rgb_loss(torch.flip(probs, [2]), vrgb, images, f)

    def rgb_new_fwd():
        with torch.no_grad():
            return R.drc_rgb_loss(cfg_c, rgb_outputs(), rgb, images, kern_c, grids=grids)

    def rgb_composed_fwd():
        with torch.no_grad():
            return composed_rgb_loss()

    def rgb_new_both():
        vox.grad = C.grad = None
        R.drc_rgb_loss(cfg_c, rgb_outputs(), rgb, images, kern_c, grids=grids).backward()

    def rgb_composed_both():
        vox.grad = C.grad = None
        composed_rgb_loss().backward()

    fns = {"mask_new_forward_ms": mask_new_fwd, "mask_composed_forward_ms": mask_composed_fwd,
           "mask_new_forward_backward_ms": mask_new_both, "mask_composed_forward_backward_ms": mask_composed_both,
           "rgb_new_forward_ms": rgb_new_fwd, "rgb_composed_forward_ms": rgb_composed_fwd,
           "rgb_new_forward_backward_ms": rgb_new_both, "rgb_composed_forward_backward_ms": rgb_composed_both}
    if a.route != "both":
        fns = {k: v for k, v in fns.items() if "_%s_" % a.route in k}
    # the two routes compute the same thing: max differences at the timed size
    agree = None
    if a.route == "both":
        def rel(x, y):
            return float((x - y).abs().max()) / max(1.0, float(y.abs().max()))

        mask_new_both()
        g_new, s_new, l_new = grid.grad.clone(), sl.grad.clone(), float(mask_new_fwd())
        mask_composed_both()
        # the lazy route's D pass keeps all 21 taps, the column kernels the 7 that matter in fp32: voxels whose s v sits within
        # ~1e-9 of the clamp at eps are decided differently (tools/bench_depth_loss.py has the reference); counted here
        diff, scale = (g_new - grid.grad).abs(), max(1.0, float(grid.grad.abs().max()))
        agree = {"mask_loss_rel_diff": abs(l_new - float(mask_composed_fwd())) / abs(l_new),
                 "mask_dgrid_max_abs_diff_over_scale": float(diff.max()) / scale,
                 "mask_dgrid_voxels": diff.numel(), "mask_dgrid_voxels_off_by_1e-5_scale": int((diff > 1e-5 * scale).sum()),
                 "mask_ds_max_abs_diff_over_scale": rel(s_new, sl.grad)}
        rgb_new_both()
        v_new, c_new, l_new = vox.grad.clone(), C.grad.clone(), float(rgb_new_fwd())
        rgb_composed_both()
        vdiff, vscale = (v_new - vox.grad).abs(), max(1.0, float(vox.grad.abs().max()))
        agree.update({"rgb_loss_rel_diff": abs(l_new - float(rgb_composed_fwd())) / abs(l_new),
                      "rgb_dvox_max_abs_diff_over_scale": float(vdiff.max()) / vscale,
                      "rgb_dvox_voxels_off_by_1e-5_scale": int((vdiff > 1e-5 * vscale).sum()),
                      "rgb_dC_max_abs_diff_over_scale": rel(c_new, C.grad)})
    med, spread = BL.event_windows(fns, a.reps, a.warmup, a.windows)
    grid_mb = B * G * G * G * 4 / 1e6
    # what each column kernel must move, from the shapes: grids in and out, ground truth read at the projection's size
    bytes_mb = {"k_drcmask_fwd": round(grid_mb + B * G * G * 4 / 1e6, 1), "k_drcmask_bwd": round(2 * grid_mb + B * G * G * 4 / 1e6, 1),
                "k_drcrgb_fwd": round(5 * grid_mb + B * G * G * 12 / 1e6, 1), "k_drcrgb_bwd": round(9 * grid_mb + B * G * G * 12 / 1e6, 1)}
    res = {"bench": "drc_loss", "clouds": B, "points": N, "grid": G, "gt_factor": f, "sigma_rel": 0.64, "taps_mask": 21,
           "taps_rgb": 11, "divide_by_occupancies": True, "reps": a.reps, "warmup": a.warmup, "windows": a.windows,
           "route": a.route, "timing": "device events, median window", "grid_mb": round(grid_mb, 1),
           "kernel_bytes_mb": bytes_mb, **med,
           "spread_ms": spread,
           "device": torch.cuda.get_device_name(0)}
    if a.route == "both":
        for case in ("mask", "rgb"):
            for what in ("forward", "forward_backward"):
                res["speedup_%s_%s" % (case, what)] = round(med["%s_composed_%s_ms" % (case, what)] / med["%s_new_%s_ms" % (case, what)], 2)
        res["agreement"] = agree
    BL.emit(res, a.out)


if __name__ == "__main__":
    main()
