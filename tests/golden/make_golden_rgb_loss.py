#!/usr/bin/env python3
"""Generate tests/golden/f21_rgb_loss.npz: the colour projection and its loss from the REFERENCE's own functions on CPU
where they run, and from numpy restatements of its TF-1 lines where they do not.

The reference's own, imported and called:
    util.point_cloud_to.pointcloud2voxels3d_fast(cfg, tr, None)   the occupancy splat; it pins the scatter's cells and
                                                                    weights: the numpy colour scatter with rgb == 1 must
                                                                    reproduce it in every channel
    util.point_cloud_to.smoothen_voxels3d                          per colour channel (what convolve_rgb does), and on the
                                                                    raw occupancies for the division
    util.drc.drc_projection                                        the ray-termination probabilities
The torch port of the colour branch crashes (point_cloud_to.py:64, drc.py:137), so these lines of the TF-1 originals are
restated in numpy, each next to the lines it restates: the rgb scatter (dpc/util/point_cloud.py:98-134), the clips, the
division and the flips (:244-262, 270-277), project_volume_rgb_integral (dpc/util/drc.py:132-142) and add_proj_rgb_loss
(dpc/util/losses.py:69-90).

Two cases, B = 2, about 60 points, a third of them in a blob one cell wide so that raw colours exceed 1:
    0: D = H = W = 8, 3 taps, pre-convolution clip and division by the occupancies, images at twice the size (f = 2)
    1: D = 10, H = W = 6, 5 x 5 x 7 taps, clip after the convolution, f = 1
(the division and the after-clip do not meet: colours divided by their occupancies are averages and never exceed 1)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rgb_loss.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import REF, make_cfg, quiet, save  # noqa: E402,F401  (reference import path and numpy shims)

import util.gauss_kernel as ref_gk  # noqa: E402
import util.point_cloud_to as ref_pc  # noqa: E402
from util.drc import drc_projection  # noqa: E402

CASES = (dict(B=2, N=60, vox_size=8, vox_size_z=-1, taps=3, taps_z=3, sigma=0.8, sigma_z=0.8, f=2, divide=True, clip_after=False),
         dict(B=2, N=63, vox_size=6, vox_size_z=10, taps=5, taps_z=7, sigma=0.6, sigma_z=0.8, f=1, divide=False, clip_after=True))


def kernels(cfg, case):
    """The reference's smoothing_kernel; with vox_size_z set its own reshape raises (gauss_kernel.py:49), so the three
    separable kernels are then laid out by hand from its gauss_kernel_1d, the z kernel with its own length and sigma."""
    if case["vox_size_z"] == -1:
        return ref_gk.smoothing_kernel(cfg, case["sigma"])
    k, kz = ref_gk.gauss_kernel_1d(case["taps"], case["sigma"]), ref_gk.gauss_kernel_1d(case["taps_z"], case["sigma_z"])
    return [k.reshape(1, 1, 1, 1, -1), k.reshape(1, 1, 1, -1, 1), kz.reshape(1, 1, -1, 1, 1)]


def points(rng, B, N, D, G):
    """Transformed points (z,y,x): a third in a blob one cell wide, a few outside the cube, the rest spread out."""
    tr = rng.uniform(-0.45, 0.45, (B, N, 3))
    nb = N // 3
    centre = rng.uniform(-0.2, 0.2, (B, 1, 3))
    tr[:, :nb] = centre + rng.uniform(-0.5, 0.5, (B, nb, 3)) / np.array([D - 1, G - 1, G - 1])
    tr[:, nb:nb + 3, rng.integers(0, 3)] = rng.uniform(0.51, 0.6, (B, 3)) * rng.choice([-1.0, 1.0], (B, 3))
    return tr


def numpy_rgb_scatter(cfg, tr, rgb, D, G):
    """dpc/util/point_cloud.py:60-136 with rgb:
        :76-77   valid = reduce_all(pc >= -half_size and pc <= half_size)
        :80-82   pc_grid = (pc + half_size) * (vox_size_tf - 1); indices_floor = floor(pc_grid)
        :91-92   r = pc_grid - indices_floor; rr = [1 - r, r]
        :99      updates_raw = rr[pos[0]][:, :, 0] * rr[pos[1]][:, :, 1] * rr[pos[2]][:, :, 2]
        :114-118 updates_rgb = updates_raw[..., None] * rgb, masked by valid, scatter_nd into [B,Dz,G,G,3]
        :126-134 the eight corners added up
    Returns the channel-last grid [B,D,G,G,3]."""
    B = tr.shape[0]
    valid = np.all((tr >= -0.5) & (tr <= 0.5), axis=-1)
    pc_grid = (tr + 0.5) * (np.array([[[D, G, G]]], dtype=np.float64) - 1)
    fl = np.floor(pc_grid)
    idx = fl.astype(np.int64)
    r = pc_grid - fl
    rr = [1.0 - r, r]
    out = np.zeros((B, D, G, G, 3))
    bb = np.broadcast_to(np.arange(B)[:, None], valid.shape)
    for k in range(2):
        for j in range(2):
            for i in range(2):
                upd = rr[k][:, :, 0] * rr[j][:, :, 1] * rr[i][:, :, 2]
                upd_rgb = upd[..., None] * rgb
                np.add.at(out, (bb[valid], idx[..., 0][valid] + k, idx[..., 1][valid] + j, idx[..., 2][valid] + i), upd_rgb[valid])
    return out


def ref_smooth(cfg, grid, kernel):
    """[B,D,H,W] float64 -> the reference's smoothen_voxels3d of it."""
    return ref_pc.smoothen_voxels3d(cfg, torch.from_numpy(grid).unsqueeze(1), kernel).squeeze(1).numpy()


def main():
    rng = np.random.default_rng(21)
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
        # the scatter's cells and weights are the reference's: unit colours reproduce its occupancy splat per channel
        ones = numpy_rgb_scatter(cfg, tr, np.ones_like(rgb), D, G)
        for c in range(3):
            assert np.abs(ones[..., c] - occ_raw).max() <= 1e-13 * max(1.0, occ_raw.max())
        raw = numpy_rgb_scatter(cfg, tr, rgb, D, G)
        assert raw.max() > 1.0, "the blob must push some raw colour above 1"
        # occupancies as pointcloud_project_fast makes them: clip, smooth (point_cloud.py:240-243)
        vox = ref_smooth(cfg, np.clip(occ_raw, 0.0, 1.0), kernel)
        # :244-247  if not cfg.pc_rgb_clip_after_conv: voxels_rgb = clip_by_value(voxels_rgb, 0, 1); convolve_rgb
        crgb = raw if cfg.pc_rgb_clip_after_conv else np.clip(raw, 0.0, 1.0)
        crgb = np.stack([ref_smooth(cfg, np.ascontiguousarray(crgb[..., c]), kernel) for c in range(3)], axis=-1)
        # :255-259  voxels_div = smoothen(stop_gradient(voxels_raw)); voxels_rgb /= voxels_div + epsilon
        if cfg.pc_rgb_divide_by_occupancies:
            crgb = crgb / (ref_smooth(cfg, occ_raw, kernel)[..., None] + cfg.pc_rgb_divide_by_occupancies_epsilon)
        # :261-262
        if cfg.pc_rgb_clip_after_conv:
            assert crgb.max() > 1.0
            crgb = np.clip(crgb, 0.0, 1.0)
        # :269-270  probabilities, flipped along the image rows;  :276  voxels_rgb flipped alike
        _, probs = drc_projection(torch.from_numpy(vox).unsqueeze(-1), cfg)
        probs = torch.flip(probs, [2]).numpy()                      # [D+1,B,H,W,1]
        voxels_rgb = crgb[:, :, ::-1]                               # [B,D,H,W,3], tf.reverse(voxels_rgb, [2])
        # drc.py:132-142  rgb -> [D,B,H,W,3], a background of ones appended, out = sum(p * rgb_full, 0)
        rgb_full = np.concatenate([voxels_rgb.transpose(1, 0, 2, 3, 4), np.ones((1, B, G, G, 3))], axis=0)
        proj_rgb = np.sum(probs * rgb_full, axis=0)                 # [B,H,W,3]
        # losses.py:74-77, 85-86: TF-1's bilinear resize_images without align_corners reads source coordinate
        # dst * in / out = f * dst, an integer: no interpolation, the pixel (f*y, f*x) itself
        images = rng.uniform(0.0, 1.0, (B, f * G, f * G, 3))
        src = np.arange(G) * (f * G / G)
        assert np.array_equal(src, np.floor(src)) and np.array_equal(src.astype(np.int64), f * np.arange(G))
        gt = images[:, src.astype(np.int64)][:, :, src.astype(np.int64)]
        loss = np.sum((gt - proj_rgb) ** 2) / 2 / B
        near = np.abs(vox[vox != 0] - eps).min(), np.abs(vox[vox != 0] - (1 - eps)).min()
        assert min(near) > 1e-8, near
        out.update({"tr%d" % n: tr, "rgb%d" % n: rgb, "vox%d" % n: vox, "images%d" % n: images, "gt_small%d" % n: gt,
                    "raw%d" % n: raw, "voxels_rgb%d" % n: np.ascontiguousarray(voxels_rgb), "proj_rgb%d" % n: proj_rgb,
                    "loss%d" % n: loss, "kxy%d" % n: kernel[0].reshape(-1).numpy(), "kz%d" % n: kernel[2].reshape(-1).numpy(), "factor%d" % n: f,
                    "vox_size%d" % n: G, "vox_size_z%d" % n: case["vox_size_z"], "divide%d" % n: case["divide"],
                    "clip_after%d" % n: case["clip_after"],
                    "div_eps%d" % n: cfg.pc_rgb_divide_by_occupancies_epsilon, "eps%d" % n: eps})
    save("f21_rgb_loss.npz", **out)


if __name__ == "__main__":
    main()
