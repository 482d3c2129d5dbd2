#!/usr/bin/env python3
"""Generate tests/golden/f22_drc_loss.npz: the two ray-consistency losses from the REFERENCE's own functions on CPU where
they run, and from numpy restatements of its TF-1 lines where they do not.

The reference's own, imported and called (through the helpers of make_golden_rgb_loss.py):
    util.point_cloud_to.pointcloud2voxels3d_fast, smoothen_voxels3d   occupancies and the smoothing of every grid
    util.drc.drc_projection                                           the ray-termination probabilities
The colour grid voxels_rgb is F21's (make_golden_rgb_loss.py: the numpy restatement of dpc/util/point_cloud.py:98-134,
244-262, pinned there against the reference's occupancy splat).  The losses exist in the TF-1 originals only; their lines
(dpc/util/losses.py:23-66, 93-110) are restated in numpy below, each next to the lines it restates.

Two cases, B = 2, the points, kernels and options of F21's two cases:
    0: D = H = W = 8, division by the occupancies, masks and images at twice the size (f = 2)
    1: D = 10, H = W = 6, clip after the convolution, f = 1 -- for the math only: the reference tiles its ground truth
       cfg.vox_size times along the ray (losses.py:25, 35), which does not broadcast against D + 1 = 11 probabilities; the
       restatement tiles D times, what those lines mean for a cubic grid

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_drc_loss.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import make_cfg, quiet, save  # noqa: E402  (reference import path and numpy shims)
from make_golden_rgb_loss import CASES, kernels, numpy_rgb_scatter, points, ref_smooth  # noqa: E402

import util.point_cloud_to as ref_pc  # noqa: E402
from util.drc import drc_projection  # noqa: E402


def subsample(gt, G, f):
    """losses.py:56-59, 100-103: TF-1's bilinear resize_images without align_corners reads source coordinate
    dst * in / out = f * dst, an integer: no interpolation, the pixel (f*y, f*x) itself."""
    src = np.arange(G) * (f * G / G)
    assert np.array_equal(src, np.floor(src)) and np.array_equal(src.astype(np.int64), f * np.arange(G))
    return gt[:, src.astype(np.int64)][:, :, src.astype(np.int64)]


def numpy_drc_loss(D, probs, gt_proj):
    """losses.py:23-29 with probs [D+1,B,H,W,1], gt_proj [B,H,W,1]:
        :24   gt_proj2 = expand_dims(gt_proj, 0)
        :25   gt_proj_fg = 1 - tile(gt_proj2, [vox_size, 1, 1, 1, 1])
        :26   gt_proj_bg = gt_proj2
        :27   psi = concat([gt_proj_fg, gt_proj_bg], 0)
        :29   reduce_sum(probs * psi)"""
    gt_proj2 = gt_proj[None]
    gt_proj_fg = 1 - np.tile(gt_proj2, [D, 1, 1, 1, 1])
    psi = np.concatenate([gt_proj_fg, gt_proj2], axis=0)
    return np.sum(probs * psi)


def numpy_drc_rgb_loss(D, G, probs, rgb, gt):
    """losses.py:32-46 with probs [D+1,B,H,W,1], rgb [B,D,H,W,3], gt [B,H,W,3]:
        :34-35  gt_vol = tile(expand_dims(gt, 1), [1, vox_size + 1, 1, 1, 1])
        :38-39  rgb_pred = concat([rgb, ones([num_samples, 1, vox_size, vox_size, 3])], 1)
        :41     probs = transpose(probs, [1, 0, 2, 3, 4])
        :43-44  psi = reduce_sum(square(gt_vol - rgb_pred), 4, keep_dims)
        :46     reduce_sum(probs * psi)"""
    gt_vol = np.tile(gt[:, None], [1, D + 1, 1, 1, 1])
    rgb_pred = np.concatenate([rgb, np.ones([rgb.shape[0], 1, G, G, 3])], axis=1)
    probs = probs.transpose(1, 0, 2, 3, 4)
    psi = np.sum(np.square(gt_vol - rgb_pred), axis=4, keepdims=True)
    return np.sum(probs * psi)


def main():
    rng = np.random.default_rng(22)
    out = {}
    for n, case in enumerate(CASES):
        cfg = make_cfg(vox_size=case["vox_size"], vox_size_z=case["vox_size_z"], pc_gauss_kernel_size=case["taps"],
                       pc_rgb_divide_by_occupancies=case["divide"], pc_rgb_clip_after_conv=case["clip_after"])
        B, N, G, f = case["B"], case["N"], case["vox_size"], case["f"]
        D = G if case["vox_size_z"] == -1 else case["vox_size_z"]
        eps = cfg.drc_logsum_clip_val
        tr = points(rng, B, N, D, G)
        rgb = rng.uniform(0.05, 0.95, (B, N, 3))
        kernel = kernels(cfg, case)
        with quiet():
            occ_raw, _ = ref_pc.pointcloud2voxels3d_fast(cfg, torch.from_numpy(tr), None)
        occ_raw = occ_raw.numpy()
        vox = ref_smooth(cfg, np.clip(occ_raw, 0.0, 1.0), kernel)                       # point_cloud.py:240-243
        raw = numpy_rgb_scatter(cfg, tr, rgb, D, G)
        crgb = raw if cfg.pc_rgb_clip_after_conv else np.clip(raw, 0.0, 1.0)           # :244-247
        crgb = np.stack([ref_smooth(cfg, np.ascontiguousarray(crgb[..., c]), kernel) for c in range(3)], axis=-1)
        div = None
        if cfg.pc_rgb_divide_by_occupancies:                                            # :255-259
            div = ref_smooth(cfg, occ_raw, kernel)
        colour = crgb                                                                   # the smoothed grid, before :255-262
        if div is not None:
            crgb = crgb / (div[..., None] + cfg.pc_rgb_divide_by_occupancies_epsilon)
        if cfg.pc_rgb_clip_after_conv:                                                  # :261-262
            assert crgb.max() > 1.0
            crgb = np.clip(crgb, 0.0, 1.0)
        _, probs = drc_projection(torch.from_numpy(vox).unsqueeze(-1), cfg)
        probs = torch.flip(probs, [2]).numpy()                                          # :269-270, [D+1,B,H,W,1]
        voxels_rgb = np.ascontiguousarray(crgb[:, :, ::-1])                             # :276, [B,D,H,W,3]
        assert abs(probs.sum(0) - 1.0).max() > 1e-6, "the e^eps factors: the probabilities do not add up to one"
        # add_drc_loss (losses.py:49-66) and add_drc_rgb_loss (:93-110), without their weights
        masks = (rng.uniform(0.0, 1.0, (B, f * G, f * G, 1)) < 0.5).astype(np.float64)
        masks[rng.uniform(0.0, 1.0, masks.shape) < 0.2] = 0.5                            # pooled masks are not 0 / 1 only
        images = rng.uniform(0.0, 1.0, (B, f * G, f * G, 3))
        loss_mask = numpy_drc_loss(D, probs, subsample(masks, G, f)) / B
        loss_rgb = numpy_drc_rgb_loss(D, G, probs, voxels_rgb, subsample(images, G, f)) / B
        near = np.abs(vox[vox != 0] - eps).min(), np.abs(vox[vox != 0] - (1 - eps)).min()
        assert min(near) > 1e-8, near
        out.update({"vox%d" % n: vox, "colour%d" % n: colour, "probs%d" % n: probs[..., 0],
                    "masks%d" % n: masks[..., 0], "images%d" % n: images, "loss_mask%d" % n: loss_mask, "loss_rgb%d" % n: loss_rgb,
                    "factor%d" % n: f, "clip_after%d" % n: case["clip_after"], "div_eps%d" % n: cfg.pc_rgb_divide_by_occupancies_epsilon,
                    "eps%d" % n: eps})
        if div is not None:
            out["div%d" % n] = div
    save("f22_drc_loss.npz", **out)


if __name__ == "__main__":
    main()
