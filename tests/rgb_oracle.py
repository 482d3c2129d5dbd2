"""fp64 restatement of the colour node (csrc/dpc_rgb.hip and its composition in dpc.render.project_rgb / proj_rgb_loss) in
plain torch; gradients by autograd.  The transform, the occupancy splat, the smoothing and the DRC probabilities are those
of oracle/dpc_oracle.py.

    tr [B,N,3] (z,y,x), rgb [B,N,3], vox [B,D,H,W], kernel (list of three 5-D kernels | None), images [S,f*H,f*W,3]
    ->  proj_rgb [B,H,W,3] (rows flipped like proj), voxels_rgb [B,D,H,W,3] (flipped along H), loss

Reference (TF-1 originals): pointcloud2voxels3d_fast's rgb half (dpc/util/point_cloud.py:98-134), the clips, the division
by the occupancies and the flip of pointcloud_project_fast (:244-262, 275-277), convolve_rgb (:148-154),
project_volume_rgb_integral (dpc/util/drc.py:132-142), add_proj_rgb_loss (dpc/util/losses.py:69-90).
"""
import torch

from oracle import dpc_oracle as O

F64 = torch.float64


def splat_rgb(cfg, tr, rgb, stop_points_gradient=False):
    """C_raw[b, c, iz+k, iy+j, ix+i] += wz[k] wy[j] wx[i] rgb[b,n,c] for every point inside [-1/2, 1/2]^3, planar
    [B,3,D,H,W] (point_cloud.py:98-134).  Cell and weights as in O.pointcloud2voxels3d_fast; a corner past the grid (a
    coordinate exactly at +1/2) is dropped, as the device does.  stop_points_gradient: the weights are constants (:112-113)."""
    D, H, W = O.grid_dims(cfg)
    B, N, _ = tr.shape
    tr, rgb = tr.to(F64), rgb.to(F64)
    inside = ((tr >= -0.5) & (tr <= 0.5)).all(-1).reshape(-1)
    dims = torch.tensor([D, H, W], dtype=F64)
    g = (tr + 0.5) * (dims - 1.0)
    cell = torch.floor(g)
    frac = (g - cell).reshape(-1, 3)[inside]
    cell = cell.detach().reshape(-1, 3).long()[inside]
    col = rgb.reshape(-1, 3)[inside]
    b = torch.arange(B).repeat_interleave(N)[inside]
    w3 = [(1.0 - frac[:, a], frac[:, a]) for a in range(3)]
    out = torch.zeros(B, 3, D, H, W, dtype=F64)
    for k in (0, 1):
        for j in (0, 1):
            for i in (0, 1):
                iz, iy, ix = cell[:, 0] + k, cell[:, 1] + j, cell[:, 2] + i
                ok = (iz < D) & (iy < H) & (ix < W)
                w = w3[0][k] * w3[1][j] * w3[2][i]
                if stop_points_gradient:
                    w = w.detach()
                for c in range(3):
                    out = out.index_put((b[ok], torch.full_like(b[ok], c), iz[ok], iy[ok], ix[ok]), (w * col[:, c])[ok],
                                        accumulate=True)
    return out


def smooth_planes(cfg, grid, kernel):
    """The separable Gaussian on every [D,H,W] plane of a [..., D, H, W] grid, W, H, D order (convolve_rgb)."""
    if kernel is None:
        return grid
    flat = grid.reshape(-1, 1, *grid.shape[-3:])
    return O.smoothen_voxels3d(cfg, flat, kernel).reshape(grid.shape)


def colour_grid(cfg, tr, rgb, kernel, parts=None):
    """The grid the integral reads, [B,3,D,H,W]: splat, pre-clip, smoothing, division, after-clip (steps 1-5).
    parts (a dict): receives the values each clip looks at, 'pre_clip' and 'after_clip' (None when that clip is off)."""
    raw = splat_rgb(cfg, tr, rgb, cfg.pc_rgb_stop_points_gradient)
    C = raw if cfg.pc_rgb_clip_after_conv else torch.clamp(raw, 0.0, 1.0)          # :245-246
    C = smooth_planes(cfg, C, kernel)
    if cfg.pc_rgb_divide_by_occupancies:                                             # :255-259
        occ, _ = O.pointcloud2voxels3d_fast(cfg, _without_face_points(tr.detach()))
        div = smooth_planes(cfg, occ, kernel)
        C = C / (div.unsqueeze(1) + cfg.get("pc_rgb_divide_by_occupancies_epsilon", 0.01))
    if parts is not None:
        parts["raw"] = raw
        parts["pre_clip"] = None if cfg.pc_rgb_clip_after_conv else raw
        parts["after_clip"] = C if cfg.pc_rgb_clip_after_conv else None
    if cfg.pc_rgb_clip_after_conv:                                                   # :261-262
        C = torch.clamp(C, 0.0, 1.0)
    return C


def _without_face_points(tr):
    """O.pointcloud2voxels3d_fast raises for a coordinate exactly at +1/2 (as the reference does); none of the test
    inputs has one, and this keeps it that way loudly."""
    assert not bool((tr == 0.5).any()), "a coordinate exactly at +1/2: the occupancy oracle cannot splat it"
    return tr


def integrate(cfg, C, vox):
    """project_volume_rgb_integral (drc.py:132-142) with the flip of the image rows (point_cloud.py:270, 276):
    proj_rgb[b, H-1-y, x, c] = sum_{k<D} p_k C[b,c,k,y,x] + p_D * 1 (a background of ones), [B,H,W,3]."""
    p = O.drc_event_probabilities(vox.to(F64).unsqueeze(-1), cfg)[..., 0]          # [D+1,B,H,W]
    proj = (p[:-1].permute(1, 0, 2, 3).unsqueeze(1) * C.to(F64)).sum(2) + p[-1].unsqueeze(1)
    return torch.flip(proj.permute(0, 2, 3, 1), [1])


def project_rgb(cfg, tr, rgb, vox, kernel, parts=None):
    """(proj_rgb [B,H,W,3], voxels_rgb [B,D,H,W,3]) -- steps 1-6."""
    C = colour_grid(cfg, tr, rgb, kernel, parts)
    return integrate(cfg, C, vox), torch.flip(C.permute(0, 2, 3, 4, 1), [2])


def subsample(images, f):
    """g[s,y,x,c] = images[s,f*y,f*x,c] for channel-last images [S,Hi,Wi,3]: the top-left pixel of every f x f window."""
    return images.to(F64)[:, ::f, ::f]


def loss_of_rgb(proj_rgb, images, f, weights=None):
    """(1/2) sum_s w_s^2 sum_{pix,c} (g - proj_rgb)^2 / S (losses.py:85-86: tf.nn.l2_loss / num_samples)."""
    sq = ((subsample(images, f) - proj_rgb.to(F64)) ** 2).sum((1, 2, 3))
    if weights is not None:
        sq = sq * weights.to(F64) ** 2
    return 0.5 * sq.sum() / proj_rgb.shape[0]


def rgb_loss(cfg, tr, rgb, vox, kernel, images, f, weights=None, parts=None):
    """(proj_rgb, voxels_rgb, loss) of the whole node -- steps 1-7."""
    proj, vrgb = project_rgb(cfg, tr, rgb, vox, kernel, parts)
    return proj, vrgb, loss_of_rgb(proj, images, f, weights)


def clip_margin(cfg, tr, rgb, vox, kernel):
    """(colour margin, DRC margin): the smallest distance of any non-zero colour value from a threshold its clip looks at,
    and of any non-zero occupancy from eps / 1 - eps.  The gradient is discontinuous at a threshold that can be crossed, so
    the parity tests assert these stay above 1e-4 / 1e-6 for their seeded inputs.
    The threshold 1 always counts.  The threshold 0 counts only when some value is negative: every colour value is a sum of
    products of non-negative weights, colours and taps -- in fp64 here and in fp32 on the device alike -- so it is either
    exactly zero (no point near) or positive on both sides of the comparison, clamp's backward passes the gradient at 0 and
    above, and that threshold cannot be crossed by rounding."""
    parts = {}
    with torch.no_grad():
        colour_grid(cfg, tr, rgb, kernel, parts)
    colour = float("inf")
    for key in ("pre_clip", "after_clip"):
        x = parts[key]
        if x is None:
            continue
        x = x.reshape(-1)
        x = x[x != 0.0]
        if x.numel():
            colour = min(colour, float((x - 1.0).abs().min()))
            if bool((x < 0).any()):
                colour = min(colour, float(x.abs().min()))
    eps = cfg.drc_logsum_clip_val
    v = vox.detach().to(F64).reshape(-1)
    v = v[v != 0.0]
    drc = float(torch.stack([(v - eps).abs().min(), (v - (1.0 - eps)).abs().min()]).min()) if v.numel() else float("inf")
    return colour, drc
