#!/usr/bin/env python3
"""Time of the k-NN search, the PCA normals and the normal-consistency metric (dpc.render.normals, csrc/dpc_knn.hip).

There is no ShapeNet on the machines this runs on, so the clouds are synthetic: per model a noisy sphere, box or torus
(tests/normals_oracle.py) as the GT cloud of --gt-points float64 points, and --views predictions of --points
float32 points each, jittered samples of the same surface.  Per k:

    knn     every prediction against itself, one dpc_knn_batched call: the wall time of knn_batched (upload included), of
            the native call alone on the packed device buffer, and k_knn's own time from the library's launch record;
            pairs per second over the kernel time and the share of the fp32 vector peak (157.3 TFLOP/s, the data sheet's,
            which counts an fma as two) at 8 unfused operations per pair (3 sub, 3 mul, 2 add; compares not counted)
    pca     dpc_pca_normals over those lists: native call and k_pca_normals' own time
    split   normal_consistency_of_split over everything (predictions' and GT normals estimated): wall time
    torch   the same rules composed from torch ops on the device (cdist squared by hand, topk, the two-pass covariance,
            torch.linalg.eigh), one cloud at a time, for --torch-clouds of the predictions; its time per cloud against
            the native k-NN + PCA time per cloud is the ratio
    numpy   tests/normals_oracle.py on the host for one cloud of --oracle-points points

and, for context only, k = 1 next to dpc_nearest_batched on the same rows.  The native lists of the torch clouds are
compared with torch's before anything is timed (where two distances tie, or differ in the last bit between the two
formulations, the lists may differ: the share of equal entries is recorded, not asserted).  One JSON line per k, appended
to profiles/normals_bench.jsonl (--out).

    python tools/bench_normals.py [--models 256] [--views 5] [--points 8000] [--gt-points 12647] [--k 8 16 30] [--reps 3]
    python tools/bench_normals.py --once                   (every workload once: for a kernel trace)
    python tools/bench_normals.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np

OPS_PER_PAIR = 8       # csrc/dpc_knn.hip pair_d2: 3 sub, 3 mul, 2 add, nothing fused


def resource_usage(path):
    BL.resource_usage("dpc_knn.hip", path, [
        "# k_knn<T, B>: lds= is the static part (the row prefix's partial sums); the lists and the tile are dynamic,",
        "# B k (sizeof(T) + 4) + 3 x 512 sizeof(T) bytes: 38 KiB (fp32) / 60 KiB (fp64) at the top of each k band"])


def clouds(a):
    """(predictions [M*V] of [points,3] float32, GT clouds [M] of [gt_points,3] float64, gt_of)."""
    import normals_oracle as G

    rng = np.random.default_rng(30)
    shapes = (G.sphere, G.box, G.torus)
    gts = [shapes[m % 3](rng, a.gt_points) + (rng.random(3) - 0.5) * 0.05 for m in range(a.models)]
    preds = np.empty((a.models * a.views, a.points, 3), dtype=np.float32)
    for m, g in enumerate(gts):
        for v in range(a.views):
            preds[m * a.views + v] = g[rng.integers(0, len(g), size=a.points)] + 0.004 * rng.normal(size=(a.points, 3))
    return preds, gts, [m for m in range(a.models) for _ in range(a.views)]


def torch_normals(P, k):
    """(idx [n,k], normals [n,3] fp64) of one cloud P [n,3] on the device by torch ops: the header's rules."""
    import torch

    d = P[None, :, :] - P[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    idx = torch.topk(d2, k, dim=1, largest=False, sorted=True).indices
    x = P.double()[idx]
    dev_ = x - x.mean(dim=1, keepdim=True)
    C = torch.einsum("qki,qkj->qij", dev_, dev_) / k
    n = torch.linalg.eigh(C).eigenvectors[:, :, 0]
    big = torch.gather(n, 1, n.abs().argmax(dim=1, keepdim=True))
    return idx, torch.where(big < 0, -n, n)


def bench(a, k, preds, gts, gt_of, torch, dev):
    import normals_oracle as O
    from dpc.render import _native, normals
    import dpc.render as R

    n_clouds, n = preds.shape[0], preds.shape[1]
    packed = torch.from_numpy(preds.reshape(-1, 3)).to(dev)
    rows = np.asarray([(i * n, n, i * n, n) for i in range(n_clouds)], dtype=np.int32)
    out = {}

    def knn_call():
        out["idx"], _, out["rows_d"] = normals._knn(packed, rows, k, dev, False)

    def pca_call():
        out["n"], _ = normals._pca(packed, rows, out["rows_d"], k, out["idx"], None, dev, False)

    knn_call()
    pca_call()
    assert R.check_status(dev) == 0
    split_in = [(preds[m * a.views:(m + 1) * a.views], None) for m in range(a.models)]
    if a.once:
        R.normal_consistency_of_split(split_in, gts, k=k)
        return None
    pairs = n_clouds * n * n
    res = {"bench": "normals", "k": k, "models": a.models, "views": a.views, "points": n, "gt_points": a.gt_points, "reps": a.reps,
           "block": _native.knn_block(k), "pairs": pairs, "ops_per_pair": OPS_PER_PAIR, "fp32_vector_peak_flops": BL.FP32_VECTOR_PEAK}
    res["knn_wall_ms_median_min_max"] = BL.median_ms(lambda: R.knn_batched(preds.reshape(-1, 3), rows, k), a.reps)
    res["knn_native_call_ms_median_min_max"] = BL.median_ms(knn_call, a.reps)
    res["pca_native_call_ms_median_min_max"] = BL.median_ms(pca_call, a.reps)
    res["kernel_ms"] = BL.kernel_ms(lambda: (knn_call(), pca_call()), dev)
    knn_s = res["kernel_ms"]["k_knn"] * 1e-3
    res["knn_pairs_per_s"] = round(pairs / knn_s, 1)
    res["knn_share_of_fp32_vector_peak"] = BL.share(pairs * OPS_PER_PAIR, res["kernel_ms"]["k_knn"], BL.FP32_VECTOR_PEAK, 4)
    res["split_wall_ms_median_min_max"] = BL.median_ms(lambda: R.normal_consistency_of_split(split_in, gts, k=k), max(1, a.reps // 2))
    # the torch composition, one cloud at a time
    t = min(a.torch_clouds, n_clouds)
    Pt = [packed[i * n:(i + 1) * n] for i in range(t)]
    same_idx, worst = [], 0.0
    for i in range(t):
        ti, tn = torch_normals(Pt[i], k)
        same_idx.append(float((ti == out["idx"][i * n:(i + 1) * n]).double().mean()))
        mine = out["n"][i * n:(i + 1) * n]
        worst = max(worst, float(torch.linalg.cross(mine, tn).norm(dim=1).median()))
    res["torch_clouds"] = t
    res["share_of_list_entries_equal_to_torch"] = round(min(same_idx), 6)
    res["median_sin_angle_to_torch_normals"] = worst
    t_ms = BL.median_ms(lambda: [torch_normals(p, k) for p in Pt], max(1, a.reps // 2))
    res["torch_ms_median_min_max"] = t_ms
    res["torch_ms_per_cloud"] = round(t_ms[0] / t, 4)
    native = (res["knn_native_call_ms_median_min_max"][0] + res["pca_native_call_ms_median_min_max"][0]) / n_clouds
    res["native_ms_per_cloud"] = round(native, 5)
    res["ratio_torch_over_native_per_cloud"] = round(t_ms[0] / t / native, 1)
    # the numpy oracle on the host, one smaller cloud
    small = preds[0][:a.oracle_points]
    t0 = time.perf_counter()
    O.estimate_normals(small, k)
    res["numpy_oracle_points"] = len(small)
    res["numpy_oracle_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["numpy_oracle_ns_per_pair"] = round(res["numpy_oracle_ms"] * 1e6 / (len(small) ** 2), 3)
    res["native_ns_per_pair"] = round(res["knn_native_call_ms_median_min_max"][0] * 1e6 / pairs, 6)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def nearest_context(a, preds, torch, dev):
    """k = 1 next to dpc_nearest_batched on the same rows (for context: that one also takes a square root per improvement
    and writes int64 indices and means)."""
    from dpc.render import _native, normals
    import dpc.render as R

    n_clouds, n = preds.shape[0], preds.shape[1]
    packed = torch.from_numpy(preds.reshape(-1, 3)).to(dev)
    rows = np.asarray([(i * n, n, i * n, n) for i in range(n_clouds)], dtype=np.int32)
    knn = BL.median_ms(lambda: normals._knn(packed, rows, 1, dev, True), a.reps)
    near = BL.median_ms(lambda: R.nearest_batched(packed, rows, return_distances=True), a.reps)
    km = BL.kernel_ms(lambda: (normals._knn(packed, rows, 1, dev, True), R.nearest_batched(packed, rows, return_distances=True)), dev)
    return {"bench": "normals_k1_context", "clouds": n_clouds, "points": n, "knn_k1_ms_median_min_max": knn,
            "nearest_batched_ms_median_min_max": near, "kernel_ms": km,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--gt-points", type=int, default=12647)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 16, 30])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-clouds", type=int, default=5)
    ap.add_argument("--oracle-points", type=int, default=2000)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "normals_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "normals_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    dev = torch.device("cuda")
    preds, gts, gt_of = clouds(a)
    for k in list(a.k) + ([] if a.once else [None]):
        res = nearest_context(a, preds, torch, dev) if k is None else bench(a, k, preds, gts, gt_of, torch, dev)
        if res is not None:
            BL.emit(res, a.out)


if __name__ == "__main__":
    main()
