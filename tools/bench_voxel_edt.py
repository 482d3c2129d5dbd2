#!/usr/bin/env python3
"""Time of the voxel distance transforms (dpc.render.voxeldist, csrc/dpc_voxel_edt.hip), stage by stage.

The grids are synthetic: balls of varying centre and radius, as solid fills and as their one-voxel shells
(voxel_shell), --grids-64 grids of 64^3 and --grids-128 grids of 128^3.  Per workload: the wall time of
voxel_distance_transform (thresholding included), of the native call alone on bit grids, and the kernels' own times from
the library's launch record, against

    torch   the same rule composed from torch ops on the device: per axis a broadcast (i - j)^2 added to the line and an
            amin over j, in int32, --torch-chunk grids at a time (the [.., n, n] array is the memory bound)
    scipy   rint(scipy.ndimage.distance_transform_edt(~grid)^2) on the host, for --host-items grids, scaled; skipped
            when scipy is not importable

Both are asserted equal to the kernels' fields before anything is timed.  Per kernel: the bytes it cannot avoid, from the
shapes -- the plane pass reads the bits and writes 4 bytes per voxel, the depth pass reads and writes 4 bytes per voxel; the
transform as a whole bits in, 4 bytes per voxel out -- over its time, as a share of the HBM peak (8.0 TB/s).  The passes are
bound by their min-plus arithmetic (two vector operations per candidate and output), and the shares say so.  Then
voxel_fscore for --models models x --views views of 64^3 against one ground truth per model: wall time and every kernel
of the call.  One JSON line per workload, appended to profiles/voxel_edt_bench.jsonl (--out).

    python tools/bench_voxel_edt.py [--grids-64 256] [--grids-128 32] [--models 256] [--views 5] [--reps 10] [--out FILE]
    python tools/bench_voxel_edt.py --once                   (every native stage once: for a kernel trace)
    python tools/bench_voxel_edt.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np

KERNELS = ("k_edt_", "k_voxel_")
INF = 1 << 28


def resource_usage(path):
    BL.resource_usage("dpc_voxel_edt.hip", path, [
        "# k_edt_plane<S, threads>: H, W <= S, LDS = 4 S^2 (g1) + 4 S S/32 (row words); k_edt_depth<S>: D <= S, LDS = 4 S 64;",
        "# all LDS is static.  The strips of k_edt_plane<128, 512> and k_edt_depth<128> hold 32 outputs in registers."])


def balls(B, G, dev, seed, jitter=0.0):
    """bool [B,G,G,G] on the device: a ball per grid, centre within 10 % of the middle, radius 25 .. 40 % of the side."""
    import torch

    rng = np.random.default_rng(seed)
    c = torch.from_numpy((0.5 + 0.1 * (rng.random((B, 3)) - 0.5) + jitter * (rng.random((B, 3)) - 0.5)) * G).to(dev).float()
    r = torch.from_numpy((0.25 + 0.15 * rng.random(B)) * G).to(dev).float()
    i = torch.arange(G, device=dev, dtype=torch.float32)
    out = torch.empty((B, G, G, G), dtype=torch.bool, device=dev)
    for b in range(B):   # one grid at a time: the fp32 temporaries of a whole batch of 128^3 are not needed
        d2 = (i[:, None, None] - c[b, 0]) ** 2 + (i[None, :, None] - c[b, 1]) ** 2 + (i[None, None, :] - c[b, 2]) ** 2
        out[b] = d2 <= r[b] ** 2
    return out


def torch_edt(occ, chunk):
    """int32 [B,D,H,W]: the three min-plus passes from broadcast adds and amin, `chunk` grids at a time."""
    import torch

    B, D, H, W = occ.shape
    out = torch.empty((B, D, H, W), dtype=torch.int32, device=occ.device)
    sqd = {}
    for n in {D, H, W}:
        i = torch.arange(n, device=occ.device, dtype=torch.int32)
        sqd[n] = (i[:, None] - i[None, :]) ** 2                      # [out, candidate]
    none = torch.full((), 2 ** 31 - 1, dtype=torch.int32, device=occ.device)
    for a in range(0, B, chunk):
        f = torch.where(occ[a:a + chunk], 0, INF).to(torch.int32)   # [b,D,H,W]
        f = (f[:, :, :, None, :] + sqd[W]).amin(-1)                  # along W: [b,D,H,w,j]
        f = (f.transpose(2, 3)[:, :, :, None, :] + sqd[H]).amin(-1).transpose(2, 3)
        f = (f.permute(0, 2, 3, 1)[:, :, :, None, :] + sqd[D]).amin(-1).permute(0, 3, 1, 2)
        out[a:a + chunk] = torch.where(f >= INF, none, f)
    return out


def bench_transform(a, G, B, kind, torch, R, dev):
    import ctypes

    from dpc.render import _native
    from dpc.render import voxeldist as VD
    from dpc.render import voxels as VX

    solid = balls(B, G, dev, G + B)
    occ = solid if kind == "solid" else R.voxel_shell(solid)
    del solid
    shape = (G, G, G)
    V, words = G ** 3, (G ** 3 + 31) // 32
    bits = VX._bits_of_grids(occ, 0.5, True, dev)
    sq = torch.empty((B,) + shape, dtype=torch.int32, device=dev)

    def native_call():
        rc = _native.lib().dpc_voxel_edt(_native.ptr(bits), B, G, G, G, 0, _native.ptr(sq), _native.stream_ptr(dev))
        _native.check(rc, "dpc_voxel_edt")

    got = R.voxel_distance_transform(occ)
    native_call()
    assert torch.equal(sq, got)
    if a.once:
        return None
    chunk = max(1, a.torch_chunk // (1 if G <= 64 else 16))
    assert torch.equal(torch_edt(occ, chunk), got), "the torch composition differs from the kernels"
    host = {"scipy": "not importable"}
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        k = min(a.host_items, B)
        grids = occ[:k].cpu().numpy()
        t0 = time.perf_counter()
        refs = [np.rint(ndimage.distance_transform_edt(~g) ** 2).astype(np.int32) for g in grids]
        ms = (time.perf_counter() - t0) * 1e3 / max(k, 1)
        assert all(np.array_equal(r, got[i].cpu().numpy()) for i, r in enumerate(refs)), "scipy differs from the kernels"
        host = {"scipy_grids_timed": k, "scipy_host_ms_per_grid": round(ms, 1), "scipy_host_ms_scaled_to_batch": round(ms * B, 1)}
    t = BL.alternate({"native_wall": lambda: R.voxel_distance_transform(occ), "native_call": native_call,
                      "torch": lambda: torch_edt(occ, chunk)}, a.reps)
    native_call()
    km = BL.kernel_ms(native_call, dev, KERNELS)
    nbytes = {"k_edt_plane": B * (words * 4 + V * 4), "k_edt_depth": B * V * 8}
    whole_ms = sum(km.get(k_, 0.0) for k_ in nbytes)
    rec = {
        "bench": "voxel_edt", "grid": G, "grids": B, "kind": kind, "reps": a.reps, "ms_median_min_max": t, "kernel_ms": km,
        "ratio_torch_over_native_call": round(t["torch"][0] / t["native_call"][0], 2),
        "ratio_torch_over_native_wall": round(t["torch"][0] / t["native_wall"][0], 2), "torch_chunk": chunk,
        "kernel_bytes": nbytes, "kernel_share_of_hbm_peak": {k_: BL.share(b, km.get(k_), BL.HBM_PEAK, 4) for k_, b in nbytes.items()},
        "transform_bytes": B * (words * 4 + V * 4), "transform_kernel_ms": round(whole_ms, 4),
        "transform_share_of_hbm_peak": BL.share(B * (words * 4 + V * 4), whole_ms, BL.HBM_PEAK, 4),
        "occupancy": round(float(occ.float().mean()), 4), "device": torch.cuda.get_device_name(0),
    }
    rec.update(host)
    if "scipy_host_ms_scaled_to_batch" in rec:
        rec["ratio_scipy_over_native_call"] = round(rec["scipy_host_ms_scaled_to_batch"] / t["native_call"][0], 1)
    return rec


def bench_fscore(a, torch, R, dev):
    M, Vw, G = a.models, a.views, 64
    gts = balls(M, G, dev, 7)
    preds = torch.empty((M * Vw, G, G, G), dtype=torch.float32, device=dev)
    for v in range(Vw):     # every view a slightly displaced copy of its model's ball
        preds[v::Vw] = balls(M, G, dev, 7, jitter=0.04 * (v + 1)).float()
    gt_of = [m for m in range(M) for _ in range(Vw)]
    taus = [0.5, 1.0, 2.0, 3.0]
    call = lambda: R.voxel_fscore(preds, gts, taus, gt_of=gt_of)
    fs = call()
    stats = R.voxel_surface_stats(preds, gts, taus, gt_of=gt_of)
    assert bool((fs[:, -1, :2] <= 1).all()) and bool((stats[:, :, 1] == stats[:, :, 0]).all())
    if a.once:
        return None
    t = BL.median_ms(call, a.reps)
    km = BL.kernel_ms(call, dev, KERNELS)
    V, words, P = G ** 3, (G ** 3 + 31) // 32, M * Vw
    nbytes = {"k_voxel_threshold": P * V * 4 + M * V + (P + M) * words * 4, "k_voxel_shell": 2 * (P + M) * words * 4,
              "k_edt_plane": (P + M) * (words * 4 + V * 4), "k_edt_depth": (P + M) * V * 8,
              "k_voxel_edt_stats": 2 * P * words * 4 + 4 * int(stats[:, :, 0].sum())}
    return {"bench": "voxel_fscore", "grid": G, "models": M, "views": Vw, "pairs": P, "thresholds": taus, "reps": a.reps,
            "ms_median_min_max": t, "kernel_ms": km, "kernel_ms_sum": round(sum(km.values()), 4), "kernel_bytes": nbytes,
            "kernel_share_of_hbm_peak": {k_: BL.share(b, km.get(k_), BL.HBM_PEAK, 4) for k_, b in nbytes.items()},
            "field_bytes": (P + M) * V * 4, "mean_f_at_1": round(float(fs[:, 1, 2].mean()), 4), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids-64", type=int, default=256)
    ap.add_argument("--grids-128", type=int, default=32)
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-items", type=int, default=2)
    ap.add_argument("--torch-chunk", type=int, default=16)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "voxel_edt_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "voxel_edt_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    import dpc.render as R

    dev = torch.device("cuda")
    for G, B in ((64, a.grids_64), (128, a.grids_128)):
        for kind in ("shell", "solid"):
            if B > 0:
                res = bench_transform(a, G, B, kind, torch, R, dev)
                if res is not None:
                    BL.emit(res, a.out)
    if a.models > 0:
        res = bench_fscore(a, torch, R, dev)
        if res is not None:
            BL.emit(res, a.out)


if __name__ == "__main__":
    main()
