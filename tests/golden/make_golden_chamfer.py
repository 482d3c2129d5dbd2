#!/usr/bin/env python3
"""Generate tests/golden/f16_chamfer_split.npz by running the REFERENCE's own Chamfer evaluation arithmetic on CPU.

F16, the Chamfer half of the evaluation (dpc/run/eval_chamfer_to.py): util.point_cloud_distance.point_cloud_distance,
util.quaternion.quaternion_rotate and util.tools.partition_range are the reference's own; compute_distance and the
per-view body of run_eval are restated line for line below (importing run/eval_chamfer_to.py itself pulls in tensorboard
and the model).  Three models of two views each:
  * m0: float32 predictions of 8500 points, the second view truncated to 7000 by num_points, a float64 GT of 9000 points:
        both directions cross numpy's 8192-element reduction buffer;
  * m1: float64 predictions of 3000 points and a float64 GT of 2000, all on a 1/32 grid with duplicated points: exact ties;
  * m2: float32 predictions of 600 points and a float32 GT of 500 with duplicates (fp32 arithmetic without a rotation).
Each model is evaluated without and with a float64 reference rotation (eval_unsupervised_shape), num_parts = 10.

The reference runs this evaluation on the GPU when it has one (device = 'cuda'), where sqrt is correctly rounded.  On the
CPU, torch's float64 sqrt is not (about 1 % of the distances here come out 1 ulp off; tests/test_gpu_parity.py's F11 test
notes the same), so point_cloud_distance is run with torch.sqrt bound to numpy's correctly rounded sqrt: everything else --
the differences, the squares, the sum over xyz, the argmin, the concatenation, np.mean, and the quaternion's norm in
quaternion_rotate -- is the reference's own CPU arithmetic.  The unpatched CPU results are stored too (chamfer_cpu_sqrt).
Stored: the clouds, chamfer [3,2,2] and final for both, and the per-point distances / indices of m0 view 0 pred -> GT.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chamfer.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import REF, save  # noqa: E402,F401  (reference import path and numpy shims)

from util.point_cloud_distance import point_cloud_distance  # noqa: E402
from util.quaternion import quaternion_rotate  # noqa: E402
from util.tools import partition_range  # noqa: E402

NUM_PARTS = 10  # cfg.pc_eval_chamfer_num_parts


def compute_distance(source_np, target_np):
    """eval_chamfer_to.py:24-44 on the CPU."""
    num_parts = NUM_PARTS
    partition = partition_range(source_np.shape[0], num_parts)
    min_dist_np = np.zeros((0,))
    idx_np = np.zeros((0,))
    source_pc = torch.from_numpy(source_np)
    target_pc = torch.from_numpy(target_np)
    for k in range(num_parts):
        r = partition[k, :]
        src = source_pc[r[0]:r[1]]
        _, min_dist, min_idx = point_cloud_distance(src, target_pc)
        min_dist_0_np = min_dist.cpu().numpy()
        idx_0_np = min_idx.cpu().numpy()
        min_dist_np = np.concatenate((min_dist_np, min_dist_0_np), axis=0)
        idx_np = np.concatenate((idx_np, idx_0_np), axis=0)
    return min_dist_np, idx_np


def run_eval(models, reference_rotation, eval_unsup, num_views):
    """The model loop of eval_chamfer_to.py:88-136 on in-memory (all_pcs, all_pcs_nums, Vgt)."""
    chamfer_dists = np.zeros((0, num_views, 2), dtype=np.float64)
    first = None
    for all_pcs, all_pcs_nums, Vgt in models:
        has_number = all_pcs_nums is not None
        chamfer_dists_current = np.zeros((num_views, 2), dtype=np.float64)
        for i in range(num_views):
            pred = all_pcs[i, :, :]
            if has_number:
                pred = pred[0:all_pcs_nums[i], :]
            if eval_unsup:
                pred = np.expand_dims(pred, 0)
                pred = quaternion_rotate(torch.from_numpy(pred), torch.from_numpy(reference_rotation)).cpu().numpy()
                pred = np.squeeze(pred)
            pred_to_gt, idx_np = compute_distance(pred, Vgt)
            gt_to_pred, _ = compute_distance(Vgt, pred)
            chamfer_dists_current[i, 0] = np.mean(pred_to_gt)
            chamfer_dists_current[i, 1] = np.mean(gt_to_pred)
            assert not np.any(np.isnan(pred_to_gt))
            if first is None:
                first = (pred_to_gt, idx_np)
        chamfer_dists = np.concatenate((chamfer_dists, np.expand_dims(chamfer_dists_current, 0)))
    final = np.mean(chamfer_dists, axis=(0, 1)) * 100
    return chamfer_dists, final, first


def shape(rng, n, dtype):
    """Points near a unit sphere shell: a shape-like cloud, not a uniform box."""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (0.4 * v * (1 + 0.05 * rng.standard_normal((n, 1)))).astype(dtype)


def main():
    rng = np.random.default_rng(16)
    V = 2
    p0 = np.stack([shape(rng, 8500, np.float32) for _ in range(V)])
    n0 = np.array([8500, 7000], dtype=np.int32)
    g0 = shape(rng, 9000, np.float64)
    grid = lambda a: np.round(a * 32) / 32
    p1 = np.stack([grid(shape(rng, 3000, np.float64)) for _ in range(V)])
    g1 = grid(shape(rng, 2000, np.float64))
    g1[1000:1200] = g1[0:200]                       # exact duplicates in the GT
    p1[0, 1500:1600] = p1[0, 0:100]
    p2 = np.stack([shape(rng, 600, np.float32) for _ in range(V)])
    p2[1, 300:350] = p2[1, 0:50]
    g2 = shape(rng, 500, np.float32)
    g2[400:450] = g2[0:50]
    q = rng.standard_normal((1, 4))                  # float64, unnormalised, as loadmat hands the rotation over
    models = [(p0, n0, g0), (p1, None, g1), (p2, None, g2)]
    chamfer_cpu_sqrt, _, _ = run_eval(models, q, False, V)
    torch_sqrt = torch.sqrt
    torch.sqrt = lambda x: torch.from_numpy(np.sqrt(x.numpy()))   # correctly rounded, as on the GPU (see above)
    try:
        chamfer, final, (d0, i0) = run_eval(models, q, False, V)
        chamfer_rot, final_rot, _ = run_eval(models, q, True, V)
    finally:
        torch.sqrt = torch_sqrt
    print("chamfer", chamfer.tolist(), "final", final.tolist(), "final_rot", final_rot.tolist())
    save("f16_chamfer_split.npz", pred0=p0, nums0=n0, gt0=g0, pred1=p1, gt1=g1, pred2=p2, gt2=g2, rotation=q,
         chamfer=chamfer, final=final, chamfer_rot=chamfer_rot, final_rot=final_rot, pair_dist=d0, pair_idx=i0,
         chamfer_cpu_sqrt=chamfer_cpu_sqrt)


if __name__ == "__main__":
    main()
