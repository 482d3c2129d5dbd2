#!/usr/bin/env python3
"""Time of the voxel-grid evaluation (dpc.render.voxels, csrc/dpc_voxels.hip) at the evaluation's shapes, stage by stage:

    split     iou_of_split: --models models x --views views of 8000 fp32 points against fp64 ground-truth clouds of 12647
              points, at 64^3 and at 128^3; its stages voxelise (predictions, ground truth) and stats timed on their own
    grids     --models * --views float32 grids of 64^3: threshold, stats against --models bool grids, and
              voxels2pc_batched at about 5 % occupancy

Each native stage is timed against the same rule composed from torch ops on the device (index arithmetic, index_put_ into
a bool grid, logical ops and sums, nonzero), alternating the two in one process, and against the numpy oracle of
tests/voxels_oracle.py on the host for --host-items items, scaled to the batch.  The results of the native path and of the
torch composition are asserted identical before anything is timed.  Per kernel: the bytes it moves, computed from the
shapes, over its time from the library's launch record, as a share of the HBM peak (8.0 TB/s).  One JSON line per stage,
appended to profiles/voxels_bench.jsonl (--out).

    python tools/bench_voxels.py [--models 256] [--views 5] [--reps 20] [--host-items 2] [--out FILE]
    python tools/bench_voxels.py --once                   (every native stage once: for a kernel trace)
    python tools/bench_voxels.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np


def resource_usage(path):
    BL.resource_usage("dpc_voxels.hip", path, [
        "# k_voxelise<fp64 input, words per workgroup, threads>; lds= is the static part, k_voxelise's bits are dynamic:",
        "# 4 bytes per word + 16, i.e. 4112, 32784 and 65552 B"])


def kernel_ms(fn, dev):
    fn()
    return BL.kernel_ms(fn, dev, "k_vox")


def share(nbytes, ms):
    return BL.share(nbytes, ms, BL.HBM_PEAK, 4)


# --- the same rules from torch ops ---------------------------------------------------------------------------------
def torch_voxelise(pts, shape):
    """pts [C,n,3] -> bool [C,V]: the nearest-node rule in fp64, index_put_ into a bool grid."""
    import torch

    C = pts.shape[0]
    D, H, W = shape
    p = pts.double()
    valid = ((p >= -0.5) & (p <= 0.5)).all(dim=2)
    scale = torch.tensor([D - 1, H - 1, W - 1], dtype=torch.float64, device=pts.device)
    idx = torch.floor((p + 0.5) * scale + 0.5).long()
    flat = (idx[..., 0] * H + idx[..., 1]) * W + idx[..., 2] + (torch.arange(C, device=pts.device) * (D * H * W))[:, None]
    grid = torch.zeros(C * D * H * W, dtype=torch.bool, device=pts.device)
    grid.index_put_((flat[valid],), torch.ones((), dtype=torch.bool, device=pts.device))
    return grid.view(C, -1), (~valid).sum(dim=1)


def torch_stats(p, g, gt_of, chunk=256):
    """bool [P,V], bool [Q,V] -> int64 [P,5], `chunk` pairs at a time (the logical ops' temporaries are pair-sized)."""
    import torch

    out = []
    for a in range(0, p.shape[0], chunk):
        x, y = p[a:a + chunk], g[gt_of[a:a + chunk]]
        out.append(torch.stack([(x ^ y).sum(1), (x & y).sum(1), (x | y).sum(1), (x & ~y).sum(1), (~x & y).sum(1)], dim=1))
    return torch.cat(out)


def torch_voxels2pc(v, thr):
    """[B,G,G,G] -> (packed xyz, counts): nonzero of v > thr and a coordinate lookup."""
    import torch

    G = v.shape[1]
    x = torch.arange(G, dtype=torch.float64, device=v.device) * (1.0 / (G - 1)) + (-0.5)
    x[G - 1] = 0.5
    nz = (v > thr).nonzero()
    return torch.stack([x[nz[:, 2]], x[nz[:, 1]], x[nz[:, 3]]], dim=1), torch.bincount(nz[:, 0], minlength=v.shape[0])


# --- stages --------------------------------------------------------------------------------------------------------
def bench_split(a, G, torch, R, O, dev):
    from dpc.render import voxels as VX

    M, V, N, NG = a.models, a.views, 8000, 12647
    shape = (G, G, G)
    words = VX._words(shape)
    rng = np.random.default_rng(G)
    pred_h = [((rng.random((V, N, 3)) * 1.04 - 0.52).astype(np.float32), None) for _ in range(M)]
    gt_h = [rng.random((NG, 3)) * 1.04 - 0.52 for _ in range(M)]
    pred_d = torch.from_numpy(np.concatenate([p for p, _ in pred_h])).to(dev)      # [M V, N, 3]
    gt_d = torch.from_numpy(np.stack(gt_h)).to(dev)                                # [M, NG, 3]
    pred_list, gt_list = VX._clouds(pred_d, "preds", "bench"), VX._clouds(gt_d, "gts", "bench")   # stacked: nothing to pack
    gt_of = np.repeat(np.arange(M), V)
    gt_of_d = torch.from_numpy(gt_of).to(dev)
    pairs = np.ascontiguousarray(np.stack([np.arange(M * V), gt_of], axis=1), dtype=np.int32)

    def native_stages():
        pb, dropped = VX._bits_of_clouds(pred_list, shape, dev, "bench")
        gb, _ = VX._bits_of_clouds(gt_list, shape, dev, "bench")
        return VX._pair_stats(pb, gb, pairs, shape), dropped

    def torch_stages():
        pg, dropped = torch_voxelise(pred_d, shape)
        gg, _ = torch_voxelise(gt_d, shape)
        return torch_stats(pg, gg, gt_of_d), dropped

    # identical results first: the split driver, the staged native path and the torch composition
    split = R.iou_of_split(pred_h, gt_h, vox_size=G)
    ns, nd = native_stages()
    ts, td = torch_stages()
    assert torch.equal(ns, ts) and torch.equal(nd.long(), td), "native and torch stats differ"
    assert split["stats"].reshape(-1, 5).tolist() == ns.cpu().tolist() and split["dropped"].reshape(-1).tolist() == nd.cpu().tolist()
    assert R.check_status() == 0
    if a.once:
        return None
    k = min(a.host_items, M)
    t0 = time.perf_counter()
    for m in range(k):
        gv = O.voxelise(gt_h[m], shape)[0]
        for i in range(V):
            assert O.stats(O.voxelise(pred_h[m][0][i], shape)[0], gv).tolist() == split["stats"][m, i].tolist()
    host_ms = (time.perf_counter() - t0) * 1e3 / max(k, 1)

    pb, _ = VX._bits_of_clouds(pred_list, shape, dev, "bench")
    gb, _ = VX._bits_of_clouds(gt_list, shape, dev, "bench")
    pg, _ = torch_voxelise(pred_d, shape)
    gg, _ = torch_voxelise(gt_d, shape)
    t = BL.alternate({
        "native_split": lambda: R.iou_of_split(pred_h, gt_h, vox_size=G),
        "native_stages": native_stages, "torch_stages": torch_stages,
        "native_voxelise_pred": lambda: VX._bits_of_clouds(pred_list, shape, dev, "bench"),
        "torch_voxelise_pred": lambda: torch_voxelise(pred_d, shape),
        "native_voxelise_gt": lambda: VX._bits_of_clouds(gt_list, shape, dev, "bench"),
        "torch_voxelise_gt": lambda: torch_voxelise(gt_d, shape),
        "native_stats": lambda: VX._pair_stats(pb, gb, pairs, shape),
        "torch_stats": lambda: torch_stats(pg, gg, gt_of_d),
    }, a.reps)
    del pg, gg
    km = kernel_ms(native_stages, dev)
    slabs = -(-words // 16384) if words > 8192 else 1
    vox_bytes = M * V * (N * 12 * slabs + words * 4) + M * (NG * 24 * slabs + words * 4)
    stats_bytes = M * V * words * 4 + M * words * 4 + M * V * 40     # every prediction grid once, every GT grid once from HBM
    return {
        "bench": "voxels_split", "grid": G, "models": M, "views": V, "pred_points": N, "gt_points": NG, "reps": a.reps,
        "ms_median_min_max": t, "kernel_ms": km,
        "ratio_torch_over_native": {s: round(t["torch_" + s][0] / t["native_" + s][0], 2)
                                    for s in ("stages", "voxelise_pred", "voxelise_gt", "stats")},
        "kernel_bytes": {"k_voxelise": vox_bytes, "k_voxel_stats": stats_bytes},
        "kernel_share_of_hbm_peak": {"k_voxelise": share(vox_bytes, km.get("k_voxelise")),
                                     "k_voxel_stats": share(stats_bytes, km.get("k_voxel_stats"))},
        "numpy_models_timed": k, "numpy_host_ms_per_model": round(host_ms, 1), "numpy_host_ms_scaled_to_batch": round(host_ms * M, 1),
        "mean_iou": float(np.nanmean(split["iou"])), "dropped_per_view": float(split["dropped"].mean()),
        "device": torch.cuda.get_device_name(0),
    }


def bench_grids(a, torch, R, O, dev):
    from dpc.render import voxels as VX

    M, P, G = a.models, a.models * a.views, 64
    shape, vox, words = (G, G, G), G ** 3, VX._words((G, G, G))
    gen = torch.Generator(device=dev).manual_seed(3)
    v = torch.rand((P, G, G, G), generator=gen, device=dev, dtype=torch.float32)
    v = torch.where(torch.rand((P, G, G, G), generator=gen, device=dev) < 0.05, 0.5 + 0.5 * v, 0.45 * v)   # about 5 % above 0.5
    v[:, 0, 0, :3] = torch.tensor([0.5, 0.3, float("nan")], device=dev)
    gt = torch.rand((M, G, G, G), generator=gen, device=dev) < 0.05
    gt_of = np.repeat(np.arange(M), a.views)
    gt_of_d = torch.from_numpy(gt_of).to(dev)
    pairs = np.ascontiguousarray(np.stack([np.arange(P), gt_of], axis=1), dtype=np.int32)

    pb = VX._bits_of_grids(v, 0.5, True, dev)
    gb = VX._bits_of_grids(gt, 0.0, True, dev)
    occ = v >= 0.5
    gflat = gt.view(M, -1)
    assert torch.equal(VX._unpack(pb, shape), occ) and torch.equal(VX._unpack(gb, shape), gt), "threshold differs from torch"
    ns = R.voxel_stats(v, gt, gt_of=gt_of.tolist(), threshold=0.5)
    assert torch.equal(ns, torch_stats(occ.view(P, -1), gflat, gt_of_d)), "native and torch stats differ"
    pts = R.voxels2pc_batched(v, 0.5)
    txyz, tcounts = torch_voxels2pc(v, 0.5)
    assert [len(p) for p in pts] == tcounts.cpu().tolist() and torch.equal(torch.cat(pts), txyz), "voxel2pc differs from torch"
    assert R.check_status() == 0
    if a.once:
        return None
    n_pts = int(tcounts.sum())
    k = min(a.host_items, P)
    vh = v[:k].cpu().numpy()
    gh = gt.cpu().numpy()
    t0 = time.perf_counter()
    for i in range(k):
        assert O.stats(O.threshold(vh[i], 0.5, True), gh[gt_of[i]]).tolist() == ns[i].cpu().tolist()
        assert O.voxel2pc(vh[i], 0.5)[0].tobytes() == pts[i].cpu().numpy().tobytes()
    host_ms = (time.perf_counter() - t0) * 1e3 / max(k, 1)
    t = BL.alternate({
        "native_threshold": lambda: VX._bits_of_grids(v, 0.5, True, dev), "torch_threshold": lambda: v >= 0.5,
        "native_stats": lambda: VX._pair_stats(pb, gb, pairs, shape), "torch_stats": lambda: torch_stats(occ.view(P, -1), gflat, gt_of_d),
        "native_threshold_stats": lambda: R.voxel_stats(v, gt, gt_of=gt_of.tolist(), threshold=0.5),
        "torch_threshold_stats": lambda: torch_stats((v >= 0.5).view(P, -1), gflat, gt_of_d),
        "native_voxels2pc": lambda: R.voxels2pc_batched(v, 0.5), "torch_voxels2pc": lambda: torch_voxels2pc(v, 0.5),
    }, a.reps)
    km = kernel_ms(lambda: (R.voxel_stats(v, gt, gt_of=gt_of.tolist(), threshold=0.5), R.voxels2pc_batched(v, 0.5)), dev)
    # k_voxel_threshold ran three times in that call (predictions twice: stats and voxel2pc; ground truth once, 1 byte a voxel)
    nbytes = {"k_voxel_threshold": 2 * P * (vox * 4 + words * 4) + M * (vox + words * 4),
              "k_voxel_stats": P * words * 4 + M * words * 4 + P * 40, "k_voxel_count": P * words * 4 + P * 4,
              "k_voxel2pc": P * words * 4 + n_pts * 24}
    return {
        "bench": "voxels_grids", "grid": G, "grids": P, "gt_grids": M, "occupancy": round(n_pts / (P * vox), 4), "points": n_pts,
        "reps": a.reps, "ms_median_min_max": t, "kernel_ms": km,
        "ratio_torch_over_native": {s: round(t["torch_" + s][0] / t["native_" + s][0], 2)
                                    for s in ("threshold", "stats", "threshold_stats", "voxels2pc")},
        "kernel_bytes": nbytes, "kernel_share_of_hbm_peak": {k_: share(b, km.get(k_)) for k_, b in nbytes.items()},
        "numpy_items_timed": k, "numpy_host_ms_per_grid": round(host_ms, 1), "numpy_host_ms_scaled_to_batch": round(host_ms * P, 1),
        "device": torch.cuda.get_device_name(0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-items", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "voxels_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "voxels_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    import dpc.render as R
    import voxels_oracle as O

    dev = torch.device("cuda")
    lines = [bench_split(a, 64, torch, R, O, dev), bench_split(a, 128, torch, R, O, dev), bench_grids(a, torch, R, O, dev)]
    for res in lines:
        if res is not None:
            BL.emit(res, a.out)


if __name__ == "__main__":
    main()
