#!/usr/bin/env python3
"""Time of the Chamfer loss (dpc.render.chamfer_loss: forward, and forward + backward) at a training-batch shape, against a
plain torch autograd brute force of one pair on the same GPU scaled to the batch.  Prints one JSON line and appends it to
profiles/chamfer_loss_bench.jsonl (--out).

The shape: 32 predictions of 8 000 float32 points against 32 GT clouds, both directions.  The GT clouds are ASSUMED to hold
16 384 points (float32 here, as a training loader would hand them over): their real size is not known (the same assumption
as tools/bench_chamfer.py and tools/bench_icp.py), and the cost scales linearly with it.

    python tools/bench_chamfer_loss.py [--pairs 32] [--n-pred 8000] [--n-gt 16384] [--reps 20] [--torch-reps 3] [--squared]
                                       [--out FILE]

kernel_ms_*: the library's own event timing of one call (dpc_profile_enable), summed per kernel; the backward's kernels
(k_chamfer_bwd_*) are to be read against the forward's k_chamfer_partial of the same run."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np
import torch

import dpc.render as R
from dpc.render import _native
from bench_chamfer import shape_cloud


def torch_pair(pred, gt, squared):
    """The brute force a user would write: [Ns,Nt,3] differences, both directions of one pair."""
    d = torch.sqrt(((gt[None, :, :] - pred[:, None, :]) ** 2).sum(2))
    a, b = d.min(dim=1).values, d.min(dim=0).values
    return ((a * a).mean() + (b * b).mean()) if squared else (a.mean() + b.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--n-pred", type=int, default=8000)
    ap.add_argument("--n-gt", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--squared", action="store_true")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "chamfer_loss_bench.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    preds = torch.from_numpy(np.stack([shape_cloud(a.n_pred, rng) for _ in range(a.pairs)]).astype(np.float32)).to(dev)
    gts = [torch.from_numpy(shape_cloud(a.n_gt, rng).astype(np.float32)).to(dev) for _ in range(a.pairs)]
    preds.requires_grad_(True)

    def forward():
        with torch.no_grad():
            return R.chamfer_loss(preds, gts, squared=a.squared)

    def forward_backward():
        preds.grad = None
        R.chamfer_loss(preds, gts, squared=a.squared).sum().backward()

    fwd_ms = BL.batch_ms(forward, a.reps)
    both_ms = BL.batch_ms(forward_backward, a.reps)
    prof = _native.profile_kernels(forward_backward, dev)
    kern = {k: round(sum(v), 4) for k, v in prof.items()}
    bwd_kernels = sum(v for k, v in kern.items() if k.startswith("k_chamfer_bwd"))

    # plain torch autograd on one pair, scaled to the batch
    p0 = preds[0].detach().clone().requires_grad_(True)

    def torch_forward():
        with torch.no_grad():
            return torch_pair(p0, gts[0], a.squared)

    def torch_forward_backward():
        p0.grad = None
        torch_pair(p0, gts[0], a.squared).backward()

    t_fwd = t_both = diff = None
    if a.torch_reps > 0:    # --torch-reps 0: the library alone (a run under rocprofv3 --kernel-trace --stats)
        t_fwd = BL.batch_ms(torch_forward, a.torch_reps) * a.pairs
        t_both = BL.batch_ms(torch_forward_backward, a.torch_reps) * a.pairs
        # the two agree on the pair both computed
        ours = R.chamfer_loss(preds[:1].detach(), gts[:1], squared=a.squared).sum()
        diff = abs(float(ours) - float(torch_forward()))

    res = {
        "bench": "chamfer_loss", "pairs": a.pairs, "n_pred": a.n_pred, "n_gt": a.n_gt, "gt_size_assumed": True,
        "dtype": "float32", "squared": bool(a.squared), "directions": 2,
        "pair_evals": 2.0 * a.pairs * a.n_pred * a.n_gt,
        "forward_ms": round(fwd_ms, 3), "forward_backward_ms": round(both_ms, 3),
        "kernel_ms_forward_backward": kern, "kernel_ms_k_chamfer_partial": kern.get("k_chamfer_partial"),
        "kernel_ms_backward_total": round(bwd_kernels, 4),
        "device": torch.cuda.get_device_name(0),
    }
    if t_both is not None:
        res.update({"torch_bruteforce_forward_ms_scaled": round(t_fwd, 2),
                    "torch_bruteforce_forward_backward_ms_scaled": round(t_both, 2), "torch_pairs_timed": 1,
                    "speedup_forward_backward_vs_torch": round(t_both / both_ms, 2), "abs_diff_vs_torch_one_pair": diff})
    BL.emit(res, a.out)


if __name__ == "__main__":
    main()
