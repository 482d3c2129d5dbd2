#!/usr/bin/env python3
"""Time of the Earth Mover's Distance (dpc.render.emd_loss: forward, and forward + backward) at P = 32 and 256 pairs of
n = 1024 and 2048 random points, default eps, with the bidding rounds the pairs took; and, for four pairs of each size,
scipy.optimize.linear_sum_assignment on the host: its time and the excess of the device's total over its optimum.
scipy on the host is the baseline: the package had no EMD before.  Prints one JSON line per shape and appends them to
profiles/emd_bench.jsonl (--out).

    python tools/bench_emd.py [--pairs 32 256] [--points 1024 2048] [--reps 7] [--scipy-pairs 4] [--squared] [--out FILE]
    python tools/bench_emd.py --resource-usage [FILE]     (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after two warm-up calls, each call ended by a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np


def resource_usage(path):
    from dpc.render import _native

    L = _native.lib()
    BL.resource_usage("dpc_emd.hip", path, [
        "# k_emd_auction: dynamic LDS, 76 bytes per point + %d: %d B at n = 1024, %d B at n = %d"
        % (L.dpc_emd_lds_bytes(2) - 152, L.dpc_emd_lds_bytes(1024), L.dpc_emd_lds_bytes(_native.DPC_EMD_MAX_POINTS), _native.DPC_EMD_MAX_POINTS)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--points", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scipy-pairs", type=int, default=4)
    ap.add_argument("--squared", action="store_true")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "emd_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "emd_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    import dpc.render as R

    dev = torch.device("cuda")
    for n in a.points:
        for P in a.pairs:
            rng = np.random.default_rng(1000 * n + P)
            pred_np = (rng.random((P, n, 3)) - 0.5).astype(np.float32)
            gt_np = (rng.random((P, n, 3)) - 0.5).astype(np.float32)
            preds = torch.from_numpy(pred_np).to(dev).requires_grad_(True)
            gts = torch.from_numpy(gt_np).to(dev)

            def forward():
                with torch.no_grad():
                    return R.emd_loss(preds, gts, squared=a.squared)

            def forward_backward():
                preds.grad = None
                R.emd_loss(preds, gts, squared=a.squared).sum().backward()

            fwd = BL.median_ms(forward, a.reps, warmup=2, digits=None)
            both = BL.median_ms(forward_backward, a.reps, warmup=2, digits=None)
            emd, asg, _, rounds = R.emd_match(preds.detach(), gts, squared=a.squared)
            rounds = rounds.cpu().numpy()
            assert R.check_status() == 0 and not bool(torch.isnan(emd).any())
            res = {
                "bench": "emd", "pairs": P, "n": n, "dtype": "float32", "squared": bool(a.squared), "eps": R.emd.DEFAULT_EPS,
                "max_rounds": R.emd.default_max_rounds(n), "reps": a.reps,
                "forward_ms": round(fwd[0], 3), "forward_ms_min_max": [round(fwd[1], 3), round(fwd[2], 3)],
                "forward_backward_ms": round(both[0], 3), "forward_backward_ms_min_max": [round(both[1], 3), round(both[2], 3)],
                "rounds_mean": round(float(rounds.mean()), 1), "rounds_max": int(rounds.max()),
                "rounds_per_point_max": round(float(rounds.max()) / n, 2),
                "device": torch.cuda.get_device_name(0),
            }
            k = min(a.scipy_pairs, P)
            if k > 0:
                from scipy.optimize import linear_sum_assignment

                host_ms, excess = [], []
                for p in range(k):
                    A, B = pred_np[p].astype(np.float64), gt_np[p].astype(np.float64)
                    t0 = time.perf_counter()
                    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
                    C = d2 if a.squared else np.sqrt(d2)
                    r, c = linear_sum_assignment(C)
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                    pi = asg[p].cpu().numpy()
                    excess.append(float(C[np.arange(n), pi].sum() - C[r, c].sum()) / n)
                res.update({"scipy_pairs_timed": k, "scipy_host_ms_per_pair": round(float(np.median(host_ms)), 2),
                            "scipy_host_ms_scaled_to_batch": round(float(np.median(host_ms)) * P, 1),
                            "excess_over_optimal_mean_max": max(excess),
                            "speedup_forward_vs_scipy_scaled": round(float(np.median(host_ms)) * P / fwd[0], 1)})
            BL.emit(res, a.out)


if __name__ == "__main__":
    main()
