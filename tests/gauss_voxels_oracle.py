"""fp64 oracle of the exact Gaussian occupancy renderer (cfg.pc_fast == false).

The reference defines it in its TF-1 original only (dpc/util/point_cloud.py:17-57 pointcloud2voxels, :219-226
pointcloud_project; the torch port calls it at model_pc_to.py:270-273 without importing it), so it is restated here line by
line, in its literal broadcast form: the meshgrid, the [B,N,G,G,G] Gaussian (in chunks of points, which changes nothing but
the peak memory), the three normalisation modes, the sum over the points and the clip.  `literal_torch` is the same lines in
torch fp64, for autograd.  Next to it the separable form the kernels compute, in the kernels' [B,D,H,W] layout, and the
analytic gradient; tests/test_gauss_voxels_host.py checks the forms against each other.

Layouts.  tf.meshgrid's default 'xy' indexing makes the literal grid's axes follow (input_pc[...,1], input_pc[...,0],
input_pc[...,2]); the kernels write [B,D,H,W] with axes following components 0, 1, 2, so literal = kernel.transpose(1, 2).
"""
import numpy as np
import torch

MAGIC = 1.78984352254   # point_cloud.py:48 (estimate_gauss_normaliser)
NONE, ANALYTICAL, PER_POINT = 0, 1, 2


def _get(cfg, key, default):
    try:
        return getattr(cfg, key)
    except (AttributeError, KeyError):
        return default


def normalise_mode(cfg):
    """point_cloud.py:43-51: pc_normalise_gauss wins, then pc_normalise_gauss_analytical (the default), then neither."""
    if _get(cfg, "pc_normalise_gauss", False):
        return PER_POINT
    return ANALYTICAL if _get(cfg, "pc_normalise_gauss_analytical", True) else NONE


def pointcloud2voxels_literal(input_pc, vox_size, sigma, mode, chunk=8):
    """point_cloud.py:17-57 with numpy fp64.  input_pc [B,N,3] -> (raw, voxels), both [B,G,G,G,1]; raw is `summed` (:53)."""
    input_pc = np.asarray(input_pc, dtype=np.float64)
    B, N = input_pc.shape[:2]
    rng = np.linspace(-1.0, 1.0, vox_size)                                   # :25
    xg, yg, zg = np.meshgrid(rng, rng, rng)                                  # :26  [G,G,G], 'xy' indexing
    xg, yg, zg = xg[None, None], yg[None, None], zg[None, None]              # :32-34
    summed = np.zeros((B, vox_size, vox_size, vox_size))
    for n0 in range(0, N, chunk):
        part = input_pc[:, n0:n0 + chunk]
        x_big = part[:, :, 0][:, :, None, None, None]                        # :19-21, 28-30
        y_big = part[:, :, 1][:, :, None, None, None]
        z_big = part[:, :, 2][:, :, None, None, None]
        sq_distance = np.square(x_big - xg) + np.square(y_big - yg) + np.square(z_big - zg)   # :37
        func = np.exp(-sq_distance / (2.0 * sigma * sigma))                  # :40  [B,n,G,G,G]
        if mode == PER_POINT:                                                # :43-45
            func = func / np.sum(func, axis=(2, 3, 4), keepdims=True)
        elif mode == ANALYTICAL:                                             # :46-51
            sigma_normalised = sigma * vox_size
            func = func * (1.0 / (MAGIC * np.power(sigma_normalised, 3)))
        summed += np.sum(func, axis=1)                                       # :53
    voxels = np.clip(summed, 0.0, 1.0)                                       # :54
    return summed[..., None], voxels[..., None]                              # :55


def literal_torch(input_pc, vox_size, sigma, mode):
    """The same lines in torch fp64 (differentiable): input_pc [B,N,3] -> (raw, voxels) [B,G,G,G,1]."""
    input_pc = input_pc.double()
    rng = torch.linspace(-1.0, 1.0, vox_size, dtype=torch.float64)
    xg, yg, zg = torch.meshgrid(rng, rng, rng, indexing="xy")
    x_big, y_big, z_big = (input_pc[:, :, a][:, :, None, None, None] for a in range(3))
    sq_distance = (x_big - xg) ** 2 + (y_big - yg) ** 2 + (z_big - zg) ** 2
    func = torch.exp(-sq_distance / (2.0 * sigma * sigma))
    if mode == PER_POINT:
        func = func / func.sum(dim=(2, 3, 4), keepdim=True)
    elif mode == ANALYTICAL:
        func = func * (1.0 / (MAGIC * (sigma * vox_size) ** 3))
    summed = func.sum(dim=1)
    return summed.unsqueeze(-1), torch.clamp(summed, 0.0, 1.0).unsqueeze(-1)


# ------------------------------------------------------------------------------------------------------
# The separable form, kernel layout: raw[b,z,y,x] = k sum_n P_0[n,z] P_1[n,y] P_2[n,x]
# ------------------------------------------------------------------------------------------------------
def scale(G, sigma, mode):
    return 1.0 / (MAGIC * (sigma * G) ** 3) if mode == ANALYTICAL else 1.0


def tables(tr, G, sigma, mode, shifted=True):
    """(P [3][B,N,G], dP [3][B,N,G]): the 1-D tables and their derivatives to the coordinate.  P_a = e_a (divided by its sum
    over the grid under PER_POINT); dP_a = P_a (w - wbar), w = -(t - c_i) / sigma^2, wbar = sum_i P_a w (PER_POINT) or 0.

    Under PER_POINT the exponent is taken minus its largest value over the grid, per point and axis: the quotient e / sum e
    is the same number, and a point whose Gaussians all underflow (exp's argument below about -745: a point well outside
    the grid under a narrow sigma) keeps its table instead of 0 / 0.  shifted=False is the quotient as the reference writes
    it, kept for tests/test_gauss_voxels_host.py to compare the two where the plain one is finite."""
    tr = np.asarray(tr, dtype=np.float64)
    c = np.linspace(-1.0, 1.0, G)
    P, dP = [], []
    for a in range(3):
        d = tr[:, :, a, None] - c
        arg = -d * d / (2.0 * sigma * sigma)
        if mode == PER_POINT and shifted:
            arg = arg - arg.max(-1, keepdims=True)
        e = np.exp(arg)
        w = -d / (sigma * sigma)
        if mode == PER_POINT:
            with np.errstate(invalid="ignore"):      # shifted=False: 0 / 0 where every Gaussian of a point underflows
                e = e / e.sum(-1, keepdims=True)
            w = w - (e * w).sum(-1, keepdims=True)
        P.append(e)
        dP.append(e * w)
    return P, dP


def raw_separable(tr, G, sigma, mode):
    """[B,D,H,W] sums before the clip, axes following components 0, 1, 2 of tr."""
    P, _ = tables(tr, G, sigma, mode)
    return scale(G, sigma, mode) * np.einsum("bnz,bny,bnx->bzyx", P[0], P[1], P[2], optimize=True)


def grad_separable(tr, G, sigma, mode, dvox, raw=None):
    """d sum(vox * dvox) / d tr, [B,N,3]: the analytic gradient through the inclusive clip mask 0 <= raw <= 1."""
    P, dP = tables(tr, G, sigma, mode)
    if raw is None:
        raw = raw_separable(tr, G, sigma, mode)
    g = np.asarray(dvox, dtype=np.float64) * ((raw >= 0.0) & (raw <= 1.0)) * scale(G, sigma, mode)
    t1 = np.einsum("bzyx,bnx->bnzy", g, P[2], optimize=True)
    t2 = np.einsum("bzyx,bnx->bnzy", g, dP[2], optimize=True)
    dz = np.einsum("bnzy,bnz,bny->bn", t1, dP[0], P[1], optimize=True)
    dy = np.einsum("bnzy,bnz,bny->bn", t1, P[0], dP[1], optimize=True)
    dx = np.einsum("bnzy,bnz,bny->bn", t2, P[0], P[1], optimize=True)
    return np.stack([dz, dy, dx], axis=-1)


def clip_margin(raw):
    """(smallest raw, smallest |raw - 1|): what decides whether the clip mask of a case can be told in fp32."""
    raw = np.asarray(raw)
    return (float(raw.min()), float(np.abs(raw - 1.0).min())) if raw.size else (0.0, 1.0)


def raw_fp32_chain(tr, G, sigma, mode):
    """What an honest fp32 implementation gives for raw, [B,D,H,W] fp32: the tables' arguments formed in fp64 and rounded
    once, exp, the normalisation and the products in fp32, and the sum over the points as one fp32 chain in index order
    (what np.cumsum(..., dtype=float32) over the points gives).  Not a model of the kernels (theirs is a chain of fused multiply-adds): it says how
    much of the parity bound fp32 itself uses up at a shape, so that a case is asserted only where a correct kernel has room."""
    tr = np.asarray(tr, dtype=np.float64)
    c = np.linspace(-1.0, 1.0, G)
    P = []
    for a in range(3):
        d = tr[:, :, a, None] - c
        arg = -d * d / (2.0 * sigma * sigma)
        if mode == PER_POINT:
            arg = arg - arg.max(-1, keepdims=True)
        e = np.exp(arg.astype(np.float32))
        if mode == PER_POINT:
            e = e / e.sum(-1, keepdims=True, dtype=np.float32)
        P.append(e)
    B, N = tr.shape[:2]
    out = np.zeros((B, G, G, G), dtype=np.float32)
    for b in range(B):
        for n in range(N):    # one fp32 addition per point and voxel, in index order
            out[b] += (P[0][b, n, :, None] * P[1][b, n])[:, :, None] * P[2][b, n]
    return np.float32(scale(G, sigma, mode)) * out


def fraction_of_bound(dev, ref, tol=1e-5):
    """max|dev - ref| as a fraction of the parity bound tol * max(1, max|ref|)."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(dev - ref).max()) / (tol * max(1.0, float(np.abs(ref).max()))) if ref.size else 0.0


# ------------------------------------------------------------------------------------------------------
# pointcloud_project (point_cloud.py:219-226) on the project's torch fp64 oracle of the transform and the DRC
# ------------------------------------------------------------------------------------------------------
def pointcloud_project(cfg, point_cloud, transform, sigma):
    """torch fp64, differentiable: (proj [B,G,G,1], voxels [B,G,G,G,1], raw [B,G,G,G,1] in the layout of `voxels`)."""
    from oracle import dpc_oracle as O

    tr_pc = O.pc_perspective_transform(cfg, point_cloud.double(), transform.double())   # :220
    raw, voxels = literal_torch(tr_pc, cfg.vox_size, sigma, normalise_mode(cfg))         # :221
    voxels = voxels.permute(0, 2, 1, 3, 4)                                               # :222
    raw = raw.permute(0, 2, 1, 3, 4)
    proj, _ = O.drc_projection(voxels, cfg)                                              # :224
    proj = torch.flip(proj, [1])                                                         # :225
    return proj, voxels, raw


SPECIAL = np.array([[0.5, -0.5, 0.25], [-0.5, 0.5, 0.5], [0.7, -0.1, -0.8], [-0.93, 0.62, 0.1],
                    [1.25, 0.0, -0.2], [0.1, -1.4, 0.3], [0.2, 0.3, 1.05]])
OUTSIDE = (4, 5, 6)     # the rows of SPECIAL beyond +-1


def points(rng, B, N, special=True):
    """Test clouds [B,N,3] fp32: most points inside the cube [-1/2,1/2]^3, and, when there is room (and unless special is
    false), some exactly on its faces, some between the cube and the grid's edge, and some beyond +-1 (no outlier filter on
    this path)."""
    tr = np.tanh(0.6 * rng.standard_normal((B, N, 3))) / 2
    if special and N >= 2 * len(SPECIAL):
        tr[:, :len(SPECIAL)] = SPECIAL
    return tr.astype(np.float32)
