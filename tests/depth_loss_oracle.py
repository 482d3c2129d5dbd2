"""fp64 restatement of the fused expected-depth node (csrc/dpc_depth.hip) in plain torch; gradients by autograd.

    grid_wh [B,D,H,W] (the grid after the clamp and the W, H passes), s [B] | None, z taps | None, depths [S,f*H,f*W],
    f, weights [S] | None  ->  depth [B,H,W] (rows flipped like proj), loss

Reference: drc_event_probabilities / drc_depth_projection (dpc/util/drc.py:48-129, 145-160), the flip of
pointcloud_project_fast (dpc/util/point_cloud_to.py:239-247) and add_proj_depth_loss (dpc/util/losses.py:113-136).
"""
import math

import torch

F64 = torch.float64


def d_pass(grid_wh, kz):
    """Zero-padded correlation along D with the z taps (point_cloud_to.py:95-97, third pass); None: no pass."""
    g = grid_wh.to(F64)
    if kz is None:
        return g
    k = torch.as_tensor(kz, dtype=F64).reshape(-1)
    n, D = k.numel(), g.shape[1]
    r = (n - 1) // 2
    padded = torch.nn.functional.pad(g, (0, 0, 0, 0, r, r))
    return sum(k[i] * padded[:, i:i + D] for i in range(n))


def pre_clamp(grid_wh, s, kz):
    """s_b v_z (v_z when there is no scale): the value the clamps look at."""
    v = d_pass(grid_wh, kz)
    return v if s is None else v * s.to(F64).reshape(-1, 1, 1, 1)


def depth_map(grid_wh, s, kz, eps=1e-5, camera_distance=2.0, max_depth=10.0):
    """Expected depth [B,H,W], rows flipped."""
    x = pre_clamp(grid_wh, s, kz)
    o = torch.clamp(x, 0.0, 1.0) if s is not None else x
    y = torch.clamp(o, eps, 1.0 - eps)
    D = y.shape[1]
    free = torch.cumprod(1.0 - y, dim=1)
    A = torch.cat([torch.ones_like(free[:, :1]), free[:, :-1]], dim=1)     # A_k = prod_{j<k} (1 - y_j)
    p = y * A
    e = math.exp(eps)
    p = torch.cat([p[:, :1] * e, p[:, 1:]], dim=1)                         # the "log-unity" rows are eps, not 0
    psi = (torch.arange(D, dtype=F64) / D - 0.5 + camera_distance).reshape(1, D, 1, 1)
    depth = (p * psi).sum(1) + e * free[:, -1] * max_depth
    return torch.flip(depth, [1])


def subsample(depths, f, max_depth=10.0, max_dataset_depth=10.0):
    """g[s,y,x] = depths[s,f*y,f*x] (TF-1 nearest neighbour, no align_corners); the dataset's background value becomes
    max_depth when the two differ (losses.py:121-127)."""
    g = depths.to(F64)[:, ::f, ::f]
    if max_depth != max_dataset_depth:
        g = torch.where(g == max_dataset_depth, torch.full_like(g, max_depth), g)
    return g


def loss_of_depth(depth, depths, f, weights=None, max_depth=10.0, max_dataset_depth=10.0):
    """(1/2) sum_s w_s^2 sum_pix (g - depth)^2 / S (losses.py:131-132: tf.nn.l2_loss / num_samples)."""
    g = subsample(depths, f, max_depth, max_dataset_depth)
    sq = ((g - depth.to(F64)) ** 2).sum((1, 2))
    if weights is not None:
        sq = sq * weights.to(F64) ** 2
    return 0.5 * sq.sum() / depth.shape[0]


def depth_loss(grid_wh, s, kz, depths, f, weights=None, eps=1e-5, camera_distance=2.0, max_depth=10.0,
               max_dataset_depth=10.0):
    """(depth [B,H,W], loss) of the whole node."""
    depth = depth_map(grid_wh, s, kz, eps, camera_distance, max_depth)
    return depth, loss_of_depth(depth, depths, f, weights, max_depth, max_dataset_depth)


def clamp_margin(grid_wh, s, kz, eps=1e-5):
    """Smallest distance of a pre-clamp value from eps, 1-eps and 1, exact zeros excepted: the gradient is discontinuous
    there, so the parity tests assert this stays above 1e-6 for their seeded inputs."""
    x = pre_clamp(grid_wh, s, kz).reshape(-1)
    x = x[x != 0.0]
    return float(torch.stack([(x - eps).abs().min(), (x - (1.0 - eps)).abs().min(), (x - 1.0).abs().min()]).min())
