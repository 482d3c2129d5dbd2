#!/usr/bin/env python3
"""Time of the colour loss (dpc.render.proj_rgb_loss: forward, and forward + backward) against the same math composed from
what the package had before it: torch index_put_ for the colour scatter, torch.clamp, Smooth.apply per channel, Drc.apply
for the ray-termination probabilities, the integral over the [D+1,B,H,W] tensor and the loss in torch, differentiated by
autograd.  Prints one JSON line per configuration and appends it to profiles/rgb_loss_bench.jsonl (--out).

The shape: B = 32 clouds of 8 000 points, 64^3 grid, 11-tap Gaussian at sigma_rel 1.5, images at twice the projection's size
(f = 2).  Configurations: the reference's defaults; pc_rgb_divide_by_occupancies; pc_rgb_clip_after_conv.  Both routes start
from the SAME projection (pointcloud_project_fast runs once, outside the timed region): its transformed points and
occupancies are leaves, and what is timed is the colour node on top of them, down to the gradients at the colours, the
transformed points and the occupancies.

    python tools/bench_rgb_loss.py [--clouds 32] [--points 8000] [--grid 64] [--reps 50] [--warmup 10] [--route both]
                                   [--config all] [--out FILE] [--deterministic [--set-replicas 4]]

GPU time by device events around `reps` back-to-back calls after `warmup` calls of the same shape; the two routes alternate
in windows.  --route new|torch with --reps small: one route alone, for a run under rocprofv3 --kernel-trace --stats.

--deterministic: the second route is not the torch composition but the package's own bit-reproducible colour splat
(cfg.pc_rgb_deterministic: 64-bit fixed-point sums), "fixed" -- the default route ("new", fp32 atomics) and "fixed" alternate
in windows on the same inputs.  Two more pairs of figures say what reading colour sets in place saves: "fixed_sets", the
deterministic route fed colour sets [clouds / set-replicas, points, 3] and a point_index [clouds, points] (a permutation per
cloud), and "replicate_rgb", the replicate_rgb call (and its autograd backward) that the default route needs in front of it
for the same sets and index.  --route new|fixed: one route alone.  Lines go to profiles/rgb_splat_fixed_bench.jsonl."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import torch

import dpc.render as R
from dpc.render._ops import Drc, Smooth, Splat

CONFIGS = {"default": {}, "divide_by_occupancies": {"pc_rgb_divide_by_occupancies": True},
           "clip_after_conv": {"pc_rgb_clip_after_conv": True}}


class Cfg(dict):
    __getattr__ = dict.__getitem__


def torch_rgb_loss(cfg, geom, tr, rgb, vox, kernel, images, f):
    """proj_rgb_loss written with torch and the stage-level nodes, as a caller had to before: no host synchronisation
    (corners past the grid and points outside the cube get weight zero at a clamped index instead of being masked out)."""
    D, H, W = geom.D, geom.H, geom.W
    B, N, _ = tr.shape
    inside = ((tr >= -0.5) & (tr <= 0.5)).all(-1)
    g = (tr + 0.5) * (torch.tensor([D, H, W], device=tr.device, dtype=tr.dtype) - 1.0)
    cell = torch.floor(g)
    frac = g - cell
    if cfg.pc_rgb_stop_points_gradient:
        frac = frac.detach()
    cell = cell.detach().long()
    w = (1.0 - frac, frac)
    bidx = torch.arange(B, device=tr.device).unsqueeze(1).expand(B, N).reshape(-1)
    C = torch.zeros(B, D, H, W, 3, device=tr.device, dtype=tr.dtype)
    for k in (0, 1):
        for j in (0, 1):
            for i in (0, 1):
                iz, iy, ix = cell[..., 0] + k, cell[..., 1] + j, cell[..., 2] + i
                ok = inside & (iz >= 0) & (iz < D) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                wt = w[k][..., 0] * w[j][..., 1] * w[i][..., 2] * ok
                C = C.index_put((bidx, iz.clamp(0, D - 1).reshape(-1), iy.clamp(0, H - 1).reshape(-1), ix.clamp(0, W - 1).reshape(-1)),
                                (wt.unsqueeze(-1) * rgb).reshape(-1, 3), accumulate=True)
    C = C.permute(0, 4, 1, 2, 3).contiguous()
    if not cfg.pc_rgb_clip_after_conv:
        C = torch.clamp(C, 0.0, 1.0)
    C = Smooth.apply(C.reshape(B * 3, D, H, W), geom).reshape(B, 3, D, H, W)
    if cfg.pc_rgb_divide_by_occupancies:
        with torch.no_grad():
            div = Smooth.apply(Splat.apply(tr.detach(), geom), geom)
        C = C / (div.unsqueeze(1) + cfg.pc_rgb_divide_by_occupancies_epsilon)
    if cfg.pc_rgb_clip_after_conv:
        C = torch.clamp(C, 0.0, 1.0)
    _, probs, _ = Drc.apply(vox, geom)                                  # [D+1,B,H,W]
    proj = (probs[:-1].permute(1, 0, 2, 3).unsqueeze(1) * C).sum(2) + probs[-1].unsqueeze(1)
    proj = torch.flip(proj.permute(0, 2, 3, 1), [1])
    return 0.5 * ((images[:, ::f, ::f] - proj) ** 2).sum() / B


def run_config(a, name, dev):
    B, N, G, f = a.clouds, a.points, a.grid, 2
    cfg = Cfg(vox_size=G, vox_size_z=-1, pc_gauss_kernel_size=11, camera_distance=2.0, focal_length=1.875,
              drc_logsum_clip_val=1e-5, max_depth=10.0, pc_rgb_stop_points_gradient=False, pc_rgb_clip_after_conv=False,
              pc_rgb_divide_by_occupancies=False, pc_rgb_divide_by_occupancies_epsilon=0.01)
    cfg.update(CONFIGS[name])
    gen = torch.Generator().manual_seed(1234)
    pc = (torch.tanh(0.5 * torch.randn(B, N, 3, generator=gen)) / 2).float().to(dev)
    q = torch.randn(B, 4, generator=gen).float().to(dev)
    s = (0.5 + 0.5 * torch.rand(B, 1, generator=gen)).float().to(dev)
    rgb = (0.05 + 0.9 * torch.rand(B, N, 3, generator=gen)).float().to(dev).requires_grad_(True)
    images = torch.rand(B, f * G, f * G, 3, generator=gen).float().to(dev)
    kernel = R.smoothing_kernel(cfg, 1.5)
    geom = R._geometry(cfg, kernel)

    # one projection; the colour node of both routes starts at its transformed points and occupancies, as leaves
    with torch.no_grad():
        base = R.pointcloud_project_fast(cfg, pc, q, None, None, kernel, scaling_factor=s)
        tr = base["tr_pc"].clone().requires_grad_(True)
        vox = base["voxels"][..., 0].clone().requires_grad_(True)
    leaves = (tr, rgb, vox)

    def outputs():
        return R.ProjectionOutputs(base["proj"], lambda: {"tr_pc": tr, "voxels": vox.unsqueeze(-1)})

    def new_loss():
        return R.proj_rgb_loss(cfg, outputs(), rgb, images, kernel)

    def torch_loss():
        return torch_rgb_loss(cfg, geom, tr, rgb, vox, kernel, images, f)

    def forward(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def both(fn):
        def run():
            for x in leaves:
                x.grad = None
            fn().backward()
        return run

    other = "fixed" if a.deterministic else "torch"
    if a.deterministic:
        det = Cfg(cfg, pc_rgb_deterministic=True)
        sets_n = B // a.set_replicas
        rgb_sets = (0.05 + 0.9 * torch.rand(sets_n, N, 3, generator=gen)).float().to(dev).requires_grad_(True)
        index = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)]).to(torch.int32).to(dev)
        leaves = leaves + (rgb_sets,)

        def other_loss():
            return R.proj_rgb_loss(det, outputs(), rgb, images, kernel)

        def sets_loss():
            return R.proj_rgb_loss(det, outputs(), rgb_sets, images, kernel, point_index=index)

        def replicate():
            return R.replicate_rgb(rgb_sets, B, index).sum()
    else:
        other_loss = torch_loss
    fns = {"new_forward_ms": forward(new_loss), other + "_forward_ms": forward(other_loss),
           "new_forward_backward_ms": both(new_loss), other + "_forward_backward_ms": both(other_loss)}
    if a.route != "both":
        fns = {k: v for k, v in fns.items() if k.startswith(a.route + "_forward")}
    elif a.deterministic:
        fns.update({"fixed_sets_forward_ms": forward(sets_loss), "fixed_sets_forward_backward_ms": both(sets_loss),
                    "replicate_rgb_forward_ms": forward(replicate), "replicate_rgb_forward_backward_ms": both(replicate)})
    agree = None
    if a.route == "both":     # the two routes compute the same thing
        fns["new_forward_backward_ms"]()
        g_new, l_new = [x.grad.clone() for x in leaves[:3]], float(fns["new_forward_ms"]())
        fns[other + "_forward_backward_ms"]()
        agree = {"loss_rel_diff": abs(l_new - float(fns[other + "_forward_ms"]())) / abs(l_new)}
        for nm, gn, x in zip(("dtr", "drgb", "dvox"), g_new, leaves):
            agree[nm + "_max_abs_diff_over_scale"] = float((gn - x.grad).abs().max()) / max(1.0, float(x.grad.abs().max()))
        if a.deterministic:   # the point of the route: the same bits from call to call
            agree["fixed_loss_bit_equal_on_repeat"] = bool(torch.equal(fns["fixed_forward_ms"](), fns["fixed_forward_ms"]()))
    med, spread = BL.event_windows(fns, a.reps, a.warmup, a.windows)
    res = {"bench": "rgb_splat_fixed" if a.deterministic else "rgb_loss", "config": name, "clouds": B, "points": N, "grid": G, "gt_factor": f, "sigma_rel": 1.5, "taps": 11,
           "reps": a.reps, "warmup": a.warmup, "windows": a.windows, "route": a.route, "timing": "device events, median window",
           "colour_grid_mb": round(B * 3 * G * G * G * 4 / 1e6, 1), "splat_atomic_mb": round(B * N * 8 * 3 * 4 / 1e6, 1),
           **({"fixed_workspace_mb": round((B * 3 * G * G * G * 8 + B * 4) / 1e6, 1), "fixed_atomic_mb": round(B * N * 8 * 3 * 8 / 1e6, 1),
               "set_replicas": a.set_replicas} if a.deterministic else {}), **med,
           "spread_ms": spread,
           "device": torch.cuda.get_device_name(0)}
    if a.route == "both":
        if not a.deterministic:
            res["speedup_forward"] = round(med["torch_forward_ms"] / med["new_forward_ms"], 2)
            res["speedup_forward_backward"] = round(med["torch_forward_backward_ms"] / med["new_forward_backward_ms"], 2)
        res["agreement"] = agree
    BL.emit(res, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--route", default="both", choices=["both", "new", "torch", "fixed"])
    ap.add_argument("--deterministic", action="store_true",
                    help="compare the default route with the bit-reproducible one (pc_rgb_deterministic) instead of with torch")
    ap.add_argument("--set-replicas", type=int, default=4, help="--deterministic: clouds per colour set of the sets figures")
    ap.add_argument("--config", default="all", choices=["all"] + list(CONFIGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(BL.ROOT, "profiles", "rgb_splat_fixed_bench.jsonl" if a.deterministic else "rgb_loss_bench.jsonl")
    if (a.route == "fixed" and not a.deterministic) or (a.route == "torch" and a.deterministic):
        ap.error("--route fixed goes with --deterministic, --route torch without it")
    if a.deterministic and (a.set_replicas < 1 or a.clouds % a.set_replicas):
        ap.error("--set-replicas must divide --clouds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rgb_loss.py measures on a GPU; none is visible")
    for name in (CONFIGS if a.config == "all" else [a.config]):
        run_config(a, name, torch.device("cuda"))


if __name__ == "__main__":
    main()
