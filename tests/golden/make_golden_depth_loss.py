#!/usr/bin/env python3
"""Generate tests/golden/f20_depth_loss.npz from the REFERENCE's own DRC functions on CPU.

F20, the expected-depth loss: util.drc.drc_projection and util.drc.drc_depth_projection are the reference's own, imported
and called in the order of pointcloud_project_fast (dpc/util/point_cloud_to.py:228-247: probabilities, flip along the image
rows, depth).  The loss is add_proj_depth_loss (dpc/util/losses.py:113-136), which is TF-1 text and cannot run here; it is
restated in numpy next to the lines it restates.  The gradient with respect to the occupancies is torch autograd through the
reference's functions, in float64.

Two grids, B = 2, D = H = W = 8 and B = 2, D = 12, H = W = 6: seeded fp64 occupancies with many exact zeros and some values
above 1 - eps.  Ground-truth depths at twice the size (f = 2), some pixels at max_dataset_depth (10) with max_depth = 7.5.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_depth_loss.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import REF, make_cfg, save  # noqa: E402,F401  (reference import path and numpy shims)

from util.drc import drc_depth_projection, drc_projection  # noqa: E402

GRIDS = ((2, 8, 8, 8), (2, 12, 6, 6))
MAX_DEPTH, MAX_DATASET_DEPTH, F = 7.5, 10.0, 2


def numpy_loss(cfg, gt, pred):
    """add_proj_depth_loss without weight_scale, gt [S,Hd,Wd], pred [S,H,W]:
        :121  if cfg.max_depth != cfg.max_dataset_depth:
        :122      gt_pos = tf.cast(tf.not_equal(gt, cfg.max_dataset_depth), tf.float32)
        :123      gt_neg = tf.cast(tf.equal(gt, cfg.max_dataset_depth), tf.float32)
        :124      gt = gt_pos * gt + gt_neg * cfg.max_depth
        :126  if gt_size != pred_size:
        :127      gt = tf.image.resize_images(gt, [pred_size, pred_size], method=tf.ResizeMethod.NEAREST_NEIGHBOR)
        :131  proj_loss = tf.nn.l2_loss(gt - pred)          # sum(t ** 2) / 2
        :132  proj_loss /= tf.to_float(num_samples)
    TF-1's nearest-neighbour resize without align_corners reads source index floor(dst * in / out) = f * dst."""
    if cfg.max_depth != cfg.max_dataset_depth:
        gt_pos = (gt != cfg.max_dataset_depth).astype(np.float64)
        gt_neg = (gt == cfg.max_dataset_depth).astype(np.float64)
        gt = gt_pos * gt + gt_neg * cfg.max_depth
    f = gt.shape[1] // pred.shape[1]
    rows = np.floor(np.arange(pred.shape[1]) * (gt.shape[1] / pred.shape[1])).astype(np.int64)
    cols = np.floor(np.arange(pred.shape[2]) * (gt.shape[2] / pred.shape[2])).astype(np.int64)
    assert np.array_equal(rows, f * np.arange(pred.shape[1]))
    gt = gt[:, rows][:, :, cols]
    return gt, np.sum((gt - pred) ** 2) / 2 / pred.shape[0]


def main():
    cfg = make_cfg(max_depth=MAX_DEPTH, max_dataset_depth=MAX_DATASET_DEPTH)
    eps = cfg.drc_logsum_clip_val
    rng = np.random.default_rng(20)
    out = dict(max_depth=MAX_DEPTH, max_dataset_depth=MAX_DATASET_DEPTH, factor=F, eps=eps,
               camera_distance=cfg.camera_distance)
    for i, (B, D, H, W) in enumerate(GRIDS):
        occ = rng.random((B, D, H, W))
        occ[rng.random(occ.shape) < 0.55] = 0.0                    # many exact zeros
        high = rng.random(occ.shape) < 0.04
        occ[high] = 1.0 - eps * rng.random(int(high.sum())) * 0.5  # above 1 - eps
        occ[0, :, 0, 0] = 0.0                                      # an empty ray
        near = np.abs(occ[occ != 0] - eps).min(), np.abs(occ[occ != 0] - (1 - eps)).min()
        assert min(near) > 1e-7, near
        depths = 1.5 + 1.5 * rng.random((B, F * H, F * W))
        depths[rng.random(depths.shape) < 0.3] = MAX_DATASET_DEPTH
        vox = torch.from_numpy(occ).unsqueeze(-1).requires_grad_(True)
        _, probs = drc_projection(vox, cfg)                        # point_cloud_to.py:228
        probs = torch.flip(probs, [2])                             # :242
        depth = drc_depth_projection(probs, cfg)                   # :247, [B,H,W,1]
        g, loss = numpy_loss(cfg, depths, depth.detach().numpy()[..., 0])
        # the same loss on the autograd tape, for the gradient
        tloss = ((torch.from_numpy(g) - depth[..., 0]) ** 2).sum() / 2 / B
        assert abs(float(tloss.detach()) - loss) <= 1e-13 * abs(loss)
        tloss.backward()
        grad = vox.grad.numpy()[..., 0]
        assert np.isfinite(grad).all() and np.count_nonzero(grad[occ == 0]) == 0
        out.update({"occ%d" % i: occ, "depths%d" % i: depths, "depth%d" % i: depth.detach().numpy()[..., 0],
                    "gt_small%d" % i: g, "loss%d" % i: loss, "grad%d" % i: grad})
    save("f20_depth_loss.npz", **out)


if __name__ == "__main__":
    main()
