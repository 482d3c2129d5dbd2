#!/usr/bin/env python3
"""Time of the exact Gaussian occupancy renderer (dpc.render.pointcloud2voxels: forward, and forward + backward) against
the same math composed in torch on the same device: three [B,N,G] tables, the [B,G^2,N] Khatri-Rao product of the z and y
tables, one batched matmul with the [B,N,G] x table (chunked over N when --chunk is given), the scale and the clip,
differentiated by autograd.  Prints one JSON line per shape and appends it to profiles/gauss_voxels_bench.jsonl (--out).

    python tools/bench_gauss_voxels.py [--clouds 32] [--points 8000] [--grids 64,32] [--sigma-rel 3.0] [--reps 50]
                                       [--warmup 5] [--windows 5] [--chunk 0] [--out FILE]
    python tools/bench_gauss_voxels.py --resource-usage [FILE]   (no device: the compiler's per-kernel resource usage)

GPU time by device events around `reps` back-to-back calls after `warmup` calls of every timed shape (code objects loaded,
the matmul library's algorithm picked, the clock ramped); the two routes alternate in windows and the median window is
reported, with the spread.  The forward's share of the fp32 peak is 2 B N G^3 / t over 157.3 TF (vector FMA = f32 MFMA on
gfx950); the operations are computed from the shapes, the backward's two products make it 4 B N G^3.  The two routes'
results are compared at the timed size before anything is timed, and a disagreement beyond the rounding of two fp32 sums over
N points (1e-4 on the grid, 1e-3 of the gradient's scale) ends the run.  A window is `reps` calls: half a second and more
for the composed route at the default shapes."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL

MAGIC = 1.78984352254


class Cfg(dict):
    __getattr__ = dict.__getitem__


def resource_usage(path):
    BL.resource_usage("dpc_gauss_voxels.hip", path, [
        "# backward: dynamic LDS, (W + 64 (W + 1) + 384 W) * 4 bytes at the compiled width W = 2 KS: 57,728 B for G <= 32, "
        "115,200 B for G <= 64"], keep="k_gauss_voxels")


def torch_voxels(tr, G, sigma, chunk):
    """The analytical-normalisation grid [B,G,G,G] composed in torch, in the kernels' layout."""
    import torch

    B, N = tr.shape[:2]
    c = torch.linspace(-1.0, 1.0, G, device=tr.device, dtype=tr.dtype)
    raw = None
    step = N if chunk <= 0 else chunk
    for n0 in range(0, N, step):
        e = torch.exp(-(tr[:, n0:n0 + step, :, None] - c) ** 2 / (2.0 * sigma * sigma))           # [B,n,3,G]
        kr = (e[:, :, 0, :, None] * e[:, :, 1, None, :]).reshape(B, -1, G * G).transpose(1, 2)   # [B,G^2,n]
        part = torch.bmm(kr, e[:, :, 2])                                                          # [B,G^2,G]
        raw = part if raw is None else raw + part
    raw = raw.reshape(B, G, G, G) * (1.0 / (MAGIC * (sigma * G) ** 3))
    return torch.clamp(raw, 0.0, 1.0)


def bench_shape(a, G):
    import torch

    import dpc.render as R

    dev = torch.device("cuda")
    B, N = a.clouds, a.points
    sigma = a.sigma_rel / G
    cfg = Cfg(vox_size=G, vox_size_z=-1, pc_normalise_gauss=False, pc_normalise_gauss_analytical=True)
    gen = torch.Generator().manual_seed(1234)
    tr = (torch.tanh(0.5 * torch.randn(B, N, 3, generator=gen)) / 2).float().to(dev).requires_grad_(True)
    dvox = torch.randn(B, G, G, G, generator=gen).float().to(dev)

    def new_fwd():
        with torch.no_grad():
            return R.pointcloud2voxels(cfg, tr, sigma)

    def composed_fwd():
        with torch.no_grad():
            return torch_voxels(tr, G, sigma, a.chunk)

    def new_both():
        tr.grad = None
        (R.pointcloud2voxels(cfg, tr, sigma)[..., 0].transpose(1, 2) * dvox).sum().backward()

    def composed_both():
        tr.grad = None
        (torch_voxels(tr, G, sigma, a.chunk) * dvox).sum().backward()

    # the two routes compute the same thing: max differences at the timed size
    v_new, v_old = new_fwd()[..., 0].transpose(1, 2), composed_fwd()
    new_both()
    g_new = tr.grad.clone()
    composed_both()
    g_old = tr.grad.clone()
    agree = {"vox_max_abs_diff": float((v_new - v_old).abs().max()),
             "dtr_max_abs_diff_over_scale": float((g_new - g_old).abs().max()) / max(1.0, float(g_old.abs().max())),
             "clipped_fraction": float((v_old >= 1.0).float().mean())}
    # both routes are fp32 sums over N points: they agree to the rounding of those sums, or nothing is timed
    if agree["vox_max_abs_diff"] > 1e-4 or agree["dtr_max_abs_diff_over_scale"] > 1e-3:
        raise SystemExit("the two routes disagree at G = %d: %s" % (G, json.dumps(agree)))
    fns = {"new_forward_ms": new_fwd, "composed_forward_ms": composed_fwd, "new_forward_backward_ms": new_both,
           "composed_forward_backward_ms": composed_both}
    med, spread = BL.event_windows(fns, a.reps, a.warmup, a.windows)
    flop_fwd = 2.0 * B * N * G ** 3
    fwd_tf = flop_fwd / (med["new_forward_ms"] * 1e-3) / 1e12
    both_tf = 3.0 * flop_fwd / (med["new_forward_backward_ms"] * 1e-3) / 1e12
    res = {"bench": "gauss_voxels", "clouds": B, "points": N, "grid": G, "sigma_rel": a.sigma_rel, "normalise": "analytical",
           "reps": a.reps, "warmup": a.warmup, "windows": a.windows, "composed_chunk": a.chunk,
           "timing": "device events, median window", **med,
           "spread_ms": spread,
           "forward_gflop": round(flop_fwd / 1e9, 1), "new_forward_tflops": round(fwd_tf, 1),
           "new_forward_fraction_of_fp32_peak": round(fwd_tf * 1e12 / BL.FP32_VECTOR_PEAK, 3),
           "new_forward_backward_tflops": round(both_tf, 1),
           "new_forward_backward_fraction_of_fp32_peak": round(both_tf * 1e12 / BL.FP32_VECTOR_PEAK, 3),
           "speedup_forward": round(med["composed_forward_ms"] / med["new_forward_ms"], 2),
           "speedup_forward_backward": round(med["composed_forward_backward_ms"] / med["new_forward_backward_ms"], 2),
           "agreement": agree, "device": torch.cuda.get_device_name(0)}
    BL.emit(res, a.out)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--grids", default="64,32")
    ap.add_argument("--sigma-rel", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=0, help="points per matmul of the composed route (0: all at once)")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "gauss_voxels_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "gauss_voxels_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_gauss_voxels.py times kernels on an MI355X: no HIP device here")
    for G in (int(g) for g in a.grids.split(",")):
        bench_shape(a, G)


if __name__ == "__main__":
    main()
