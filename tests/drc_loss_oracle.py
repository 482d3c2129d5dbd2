"""fp64 restatement of the two ray-consistency losses (csrc/dpc_drc_loss.hip) in plain torch; gradients by autograd.

    mask loss    grid_wh [B,D,H,W], s [B] | None, z taps | None, masks [S,f*H,f*W], f, weights [S] | None   -> loss
    colour loss  vox [B,D,H,W], C [B,3,D,H,W], div [B,D,H,W] | None, images [S,f*H,f*W,3], f, weights      -> loss

Reference (TF-1 originals): drc_loss, drc_rgb_loss, add_drc_loss, add_drc_rgb_loss (dpc/util/losses.py:23-66, 93-110) on the
probabilities of drc_event_probabilities (dpc/util/drc.py:48-106) and the flips of pointcloud_project_fast
(dpc/util/point_cloud.py:269-276).  The D pass and the values the clamps look at are those of tests/depth_loss_oracle.py.
"""
import math

import torch

import depth_loss_oracle as DO

F64 = torch.float64


def probabilities(y, eps=1e-5):
    """drc_event_probabilities (drc.py:48-106, drc_logsum, drc_tf_cumulative) of occupancies y [B,D,H,W] -> [B,D+1,H,W]:
        :57       input = clamp(input, eps, 1 - eps)
        :62-66    y = log(input), x = log(1 - input)
        :80       r = cumsum(x)                                 log prod_{j<=k} (1 - y_j)
        :96-97    p1 = [eps, r]                                 log_unity is eps, not 0: the first event gets a factor e^eps
        :99-100   p2 = [y, eps]                                 ... and so does the last
        :102-104  p = exp(p1 + p2)
    i.e. p_0 = e^eps y_0, p_k = y_k prod_{j<k} (1 - y_j), p_D = e^eps prod_j (1 - y_j)."""
    y = torch.clamp(y.to(F64), eps, 1.0 - eps)
    free = torch.cumprod(1.0 - y, dim=1)
    A = torch.cat([torch.ones_like(free[:, :1]), free[:, :-1]], dim=1)
    e = math.exp(eps)
    return torch.cat([y[:, :1] * e, (y * A)[:, 1:], e * free[:, -1:]], dim=1)


def ray_probabilities(grid_wh, s, kz, eps=1e-5):
    """Probabilities [B,D+1,H,W] of the fused node's grid, rows flipped into image order (point_cloud.py:269-270):
    D pass, occupancy scale and clamp (point_cloud_to.py:218-222), then `probabilities`."""
    x = DO.pre_clamp(grid_wh, s, kz)
    o = torch.clamp(x, 0.0, 1.0) if s is not None else x
    return torch.flip(probabilities(o, eps), [2])


def weighted(per_sample, weights):
    """sum_s w_s^2 cost_s / S (losses.py:62, 106: loss /= num_samples; w the 0/1 valid_samples, squared like the other losses')."""
    if weights is not None:
        per_sample = per_sample * weights.to(F64) ** 2
    return per_sample.sum() / per_sample.shape[0]


def mask_loss_of_probabilities(p, masks, f, weights=None):
    """drc_loss + add_drc_loss (losses.py:23-29, 49-66) on probabilities p [B,D+1,H,W] in image order:
        :56-59    gt = resize_images(masks, [pred_size, pred_size])   g[y,x] = masks[f*y, f*x] for an integer factor
        :24-27    psi = [1 - g] * vox_size + [g]                      a voxel pays 1 - g, the background g
        :29       sum(probs * psi)                                    no 1/2, no square
        :62       loss /= num_samples"""
    g = masks.to(F64)[:, ::f, ::f]
    cost = ((1.0 - g) * p[:, :-1].sum(1) + g * p[:, -1]).sum((1, 2))
    return weighted(cost, weights)


def mask_loss(grid_wh, s, kz, masks, f, weights=None, eps=1e-5):
    return mask_loss_of_probabilities(ray_probabilities(grid_wh, s, kz, eps), masks, f, weights)


def colour_seen(C, div=None, div_eps=0.01, clip_after=False):
    """The colour grid the losses read, [B,3,D,H,W]: division by the occupancies and clip after the convolution
    (point_cloud.py:255-262).  Returns (value, the value the after-clip looked at | None)."""
    C = C.to(F64)
    if div is not None:
        C = C / (div.to(F64).unsqueeze(1) + div_eps)
    return (torch.clamp(C, 0.0, 1.0), C) if clip_after else (C, None)


def rgb_loss_of_probabilities(p, voxels_rgb, images, f, weights=None):
    """drc_rgb_loss + add_drc_rgb_loss (losses.py:32-46, 93-110) on probabilities p [B,D+1,H,W] and voxels_rgb [B,D,H,W,3],
    both in image order:
        :100-103  gt = resize_images(images, [pred_size, pred_size])  g[y,x,:] = images[f*y, f*x, :]
        :34-35    gt_vol = gt tiled vox_size + 1 times along the ray
        :38-39    rgb_pred = [voxels_rgb, ones]                       a white background behind the last voxel
        :43-44    psi = sum_c (gt_vol - rgb_pred)^2
        :46       sum(probs * psi);  :106  loss /= num_samples"""
    g = images.to(F64)[:, ::f, ::f].unsqueeze(1)                                  # [B,1,H,W,3]
    pred = torch.cat([voxels_rgb.to(F64), torch.ones_like(voxels_rgb[:, :1], dtype=F64)], dim=1)
    psi = ((g - pred) ** 2).sum(-1)                                               # [B,D+1,H,W]
    return weighted((p * psi).sum((1, 2, 3)), weights)


def rgb_loss(vox, C, div, images, f, weights=None, eps=1e-5, div_eps=0.01, clip_after=False):
    """The colour loss from the renderer's voxels [B,D,H,W] and the smoothed colour grid C [B,3,D,H,W] (planar), both in
    grid order: rows flipped into image order like drc_probs and voxels_rgb (point_cloud.py:269-276)."""
    p = torch.flip(probabilities(vox, eps), [2])
    seen, _ = colour_seen(C, div, div_eps, clip_after)
    return rgb_loss_of_probabilities(p, torch.flip(seen.permute(0, 2, 3, 4, 1), [2]), images, f, weights)


def clamp_margin(grid_wh, s, kz, eps=1e-5):
    """Smallest distance of a pre-clamp value s v from eps, 1 - eps and 1, exact zeros excepted (depth_loss_oracle's)."""
    return DO.clamp_margin(grid_wh, s, kz, eps)


def clip_margin(C, div=None, div_eps=0.01, clip_after=False):
    """Smallest distance of a non-zero colour value from 0 or 1 where the after-clip looks at it (inf without that clip)."""
    _, seen = colour_seen(C, div, div_eps, clip_after)
    if seen is None:
        return float("inf")
    x = seen.reshape(-1)
    x = x[x != 0.0]
    return float(torch.minimum(x.abs(), (x - 1.0).abs()).min()) if x.numel() else float("inf")
