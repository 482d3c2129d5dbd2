#!/usr/bin/env python3
"""Generate tests/golden/f27_gt_smooth.npz: ground truth resized and smoothed as cfg.pc_gauss_filter_gt asks.

The reference's own, imported and called:
    util.gauss_kernel.gauss_kernel_1d            the taps (fp32, as the reference makes them)
    torch.nn.AvgPool2d                           the mask resize of its torch port (dpc/models/model_pc_to.py:346-354)
gauss_smoothen_image itself (dpc/util/gauss_kernel.py:14-24) mixes torch.repeat and tf. calls and cannot run (the F22
precedent); its lines are restated in numpy below, each next to the line it restates.  The depth remap and the
nearest-neighbour / bilinear resizes for an integer factor exist in the TF-1 originals only (dpc/util/losses.py:74-77,
121-127) and are restated likewise.

Three cases, S = 2, everything in fp64 on the reference's fp32 taps:
    masks   [2,1,16,16] -> 8 x 8, AvgPool2d(2), 11 taps at sigma_rel = 1.0 (every pixel sees both borders)
    images  [2,6,10,3], f = 1, 5 taps at sigma_rel = 0.8 (three channels, not square)
    depths  [2,12,12,1] -> 6 x 6, max_dataset_depth 10 -> max_depth 5, pixel (2y, 2x), 7 taps at sigma_rel = 1.5

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gt_smooth.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import save  # noqa: E402  (reference import path and numpy shims)

import util.gauss_kernel as ref_gk  # noqa: E402


def numpy_depthwise_same(img, k):
    """tf.nn.depthwise_conv2d(img [S,H,W,C], k [kh,kw,C,1], [1,1,1,1], padding="SAME"): a correlation; SAME pads an odd
    kernel side n by n // 2 zeros on both sides; channel c is filtered with k[:, :, c, 0] alone."""
    S, H, W, C = img.shape
    kh, kw = k.shape[0], k.shape[1]
    ph, pw = kh // 2, kw // 2
    padded = np.zeros((S, H + 2 * ph, W + 2 * pw, C))
    padded[:, ph:ph + H, pw:pw + W] = img
    out = np.zeros_like(img)
    for s in range(S):
        for y in range(H):
            for x in range(W):
                for c in range(C):
                    out[s, y, x, c] = np.sum(padded[s, y:y + kh, x:x + kw, c] * k[:, :, c, 0])
    return out


def numpy_gauss_smoothen_image(fsz, img, sigma_rel):
    """gauss_kernel.py:14-24 with img [S,H,W,C]:
        :16     kernel = gauss_kernel_1d(fsz, sigma_rel)
        :17     in_channels = img.shape[-1]
        :18     k1 = repeat(kernel.reshape(1, fsz, 1, 1), (1, 1, in_channels, 1))
        :19     k2 = repeat(kernel.reshape((fsz, 1, 1, 1)), (1, 1, in_channels, 1))
        :22     img_tmp = depthwise_conv2d(img_tmp, k1, [1, 1, 1, 1], padding="SAME")
        :23     img_tmp = depthwise_conv2d(img_tmp, k2, [1, 1, 1, 1], padding="SAME")"""
    kernel = ref_gk.gauss_kernel_1d(fsz, sigma_rel).numpy()
    assert kernel.dtype == np.float32
    in_channels = img.shape[-1]
    k1 = np.tile(kernel.astype(np.float64).reshape(1, fsz, 1, 1), (1, 1, in_channels, 1))
    k2 = np.tile(kernel.astype(np.float64).reshape(fsz, 1, 1, 1), (1, 1, in_channels, 1))
    img_tmp = img
    img_tmp = numpy_depthwise_same(img_tmp, k1)
    img_tmp = numpy_depthwise_same(img_tmp, k2)
    return kernel, img_tmp


def subsample(gt, H, W, f):
    """losses.py:74-77, 126-127 on [S,Hs,Ws,C]: TF-1's resize_images without align_corners reads source coordinate
    dst * in / out = f * dst, an integer -- bilinear interpolates nothing there and nearest-neighbour floors nothing:
    the pixel (f*y, f*x) itself."""
    ys, xs = np.arange(H) * (f * H / H), np.arange(W) * (f * W / W)
    assert np.array_equal(ys, np.floor(ys)) and np.array_equal(xs, np.floor(xs))
    return gt[:, ys.astype(np.int64)][:, :, xs.astype(np.int64)]


def main():
    rng = np.random.RandomState(27)
    out = {}

    # masks: model_pc_to.py:346-354 (AvgPool2d(gt_size // pred_size) on [S,1,Hm,Wm]), :365 permute, model_pc.py:398-400
    masks = (rng.rand(2, 1, 16, 16) < 0.45).astype(np.float64)
    pooled = torch.nn.AvgPool2d(2)(torch.from_numpy(masks)).permute(0, 2, 3, 1).numpy()
    taps, smoothed = numpy_gauss_smoothen_image(11, pooled, 1.0)
    out.update(masks_in=masks.astype(np.float32), masks_taps=taps, masks_resized=pooled, masks_out=smoothed)

    # images: losses.py:74-83, gt already at the prediction's size
    images = rng.rand(2, 6, 10, 3)
    images = images.astype(np.float32).astype(np.float64)
    taps, smoothed = numpy_gauss_smoothen_image(5, images, 0.8)
    out.update(images_in=images.astype(np.float32), images_taps=taps, images_resized=images, images_out=smoothed)

    # depths: losses.py:121-124 (gt_pos * gt + gt_neg * max_depth where gt == max_dataset_depth), :126-129
    max_dataset_depth, max_depth = 10.0, 5.0
    depths = (1.5 + rng.rand(2, 12, 12, 1)).astype(np.float32).astype(np.float64)
    depths[rng.rand(2, 12, 12, 1) < 0.4] = max_dataset_depth
    depths[0, 4, 4, 0], depths[0, 4, 6, 0] = max_dataset_depth, 2.25   # a background pixel next to a foreground one, both sampled
    gt_pos = (depths != max_dataset_depth).astype(np.float64)
    gt_neg = (depths == max_dataset_depth).astype(np.float64)
    remapped = gt_pos * depths + gt_neg * max_depth
    small = subsample(remapped, 6, 6, 2)
    taps, smoothed = numpy_gauss_smoothen_image(7, small, 1.5)
    out.update(depths_in=depths.astype(np.float32), depths_taps=taps, depths_resized=small, depths_out=smoothed,
               depths_remap=np.array([max_dataset_depth, max_depth]))

    save("f27_gt_smooth.npz", **out)


if __name__ == "__main__":
    main()
