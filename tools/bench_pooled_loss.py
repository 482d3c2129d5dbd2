#!/usr/bin/env python3
"""What pooling the masks inside the fused loss costs: one project_loss_step per step at c2 (B = 32, N = 8000, 64^3,
sigma_rel 0.64, K = 1) and c5 (16 samples x K = 8 candidates of one shared point set each), three variants timed
alternately in one process:

  pre      the masks pooled once, outside the timed step ([S,64,64,1]: what bench.py's headline times)
  kernel   the 128^2 masks [S,1,128,128] handed to the step, pooled in the ray-march kernels -- without and with per-sample
           weights (valid_samples)
  torch    F.avg_pool2d inside the timed step, then the pre-pooled step (what a caller without in-kernel pooling runs)

Before timing, `pre` and `kernel` must give torch.equal results (loss, proj, winner, dpc, dq, ds).  Method: warm-up, then
15 windows x 200 steps per variant, each window timed with device events, the variants interleaved window by window; one
JSON line per variant: median and spread (min, max) of the per-step time in us.

    python tools/bench_pooled_loss.py [--windows 15] [--steps 200] [--configs c2,c5] [--variants pre,kernel]

(--variants: time only these, e.g. one variant per process under rocprofv3 --kernel-trace --stats for its kernel times)
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL

import dpc.render as R  # noqa: E402

CONFIGS = {"c2": dict(S=32, K=1, N=8000, G=64, shared=False), "c5": dict(S=16, K=8, N=8000, G=64, shared=True)}


class Cfg(dict):
    __getattr__ = dict.__getitem__


def setup(name, device):
    c = CONFIGS[name]
    S, K, N, G = c["S"], c["K"], c["N"], c["G"]
    B = S * K
    cfg = Cfg(vox_size=G, vox_size_z=-1, pc_gauss_kernel_size=21, camera_distance=2.0, focal_length=1.875,
              drc_logsum_clip_val=1e-5, max_depth=10.0)
    gen = torch.Generator().manual_seed(1234)
    sets = S if c["shared"] else B
    pc = (torch.tanh(0.5 * torch.randn(sets, N, 3, generator=gen)) / 2).float().to(device)
    q = torch.randn(B, 4, generator=gen).float().to(device)
    s = (0.5 + 0.5 * torch.rand(B, 1, generator=gen)).float().to(device)
    masks = (torch.rand(S, 1, 2 * G, 2 * G, generator=gen) > 0.5).float().to(device)
    weights = torch.tensor([1.0, 0.0, 0.5, 1.0] * S)[:S].to(device)
    plan = R.project_loss_step(cfg, R.smoothing_kernel(cfg, 0.64), B, N, device, num_candidates=K,
                               point_replicas=B // sets)
    return plan, pc, q, s, masks, weights


def outputs(plan):
    return tuple(x.clone() for x in (plan.loss, plan.proj, plan.winner, plan.dpc, plan.dq, plan.ds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--variants", default="pre,kernel,kernel_weighted,torch")
    args = ap.parse_args()
    device = torch.device("cuda")
    for name in args.configs.split(","):
        plan, pc, q, s, masks, w = setup(name, device)
        pre = F.avg_pool2d(masks, 2).permute(0, 2, 3, 1).contiguous()
        plan.run(pc, q, s, pre)
        a = outputs(plan)          # clones on the stream the plan ran on
        plan.run(pc, q, s, masks)
        b = outputs(plan)
        for what, x, y in zip(("loss", "proj", "winner", "dpc", "dq", "ds"), a, b):
            assert torch.equal(x, y), "%s: %s differs between pre-pooled and in-kernel pooled masks" % (name, what)
        variants = {
            "pre": lambda: plan.run(pc, q, s, pre),
            "kernel": lambda: plan.run(pc, q, s, masks),
            "kernel_weighted": lambda: plan.run(pc, q, s, masks, valid_samples=w),
            "torch": lambda: plan.run(pc, q, s, F.avg_pool2d(masks, 2).permute(0, 2, 3, 1).contiguous()),
        }
        variants = {k: variants[k] for k in args.variants.split(",")}
        times = BL.event_window_times(variants, args.steps, args.warmup, args.windows)
        for k, ms in times.items():
            t = [1e3 * x for x in ms]
            BL.emit({"tool": "bench_pooled_loss", "config": name, "variant": k, "us_per_step_median": round(statistics.median(t), 3),
                     "us_min": round(min(t), 3), "us_max": round(max(t), 3), "windows": args.windows,
                     "steps_per_window": args.steps, "bit_identical_pre_vs_kernel": True})


if __name__ == "__main__":
    main()
