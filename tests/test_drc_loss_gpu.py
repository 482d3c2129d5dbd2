"""The fused ray-consistency (DRC) mask and colour losses on the GPU (csrc/dpc_drc_loss.hip) against the fp64 oracle of
tests/drc_loss_oracle.py.

Every comparison uses the parity rule of tests/test_gpu_parity.py, max |device - reference| <= 1e-5 * max(1, max |reference|).
The gradients are discontinuous at the clamps, so every case asserts on the oracle that no pre-clamp value s v of its seeded
inputs lies within 1e-6 of eps, 1 - eps or 1 (exact zeros excepted) and, under the after-clip, that no non-zero colour lies
within 1e-6 of 0 or 1; the seeds were checked on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import drc_loss_oracle as DR
import rgb_oracle as RO
from oracle import dpc_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
EPS, MARGIN, DIV_EPS = 1e-5, 1e-6, 0.01


def dev(a, grad=False):
    t = torch.as_tensor(a).to(device="cuda", dtype=torch.float32)
    return t.requires_grad_(True) if grad else t


def close(a, b, tol=TOL, what=""):
    """The parity rule of tests/test_gpu_parity.py: max |a - b| <= tol * max(1, max |b|), b the fp64 reference."""
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    a, b = a.reshape(b.shape) if a.size == b.size else a, b
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what + ": non-finite values"
    err = float(np.abs(a - b).max()) if a.size else 0.0
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    print("%-44s max abs err %.3e  bound %.3e" % (what, err, tol * scale))
    assert err <= tol * scale, "%s: max abs err %.3e > %.1e * %.2f" % (what, err, tol, scale)


def gauss(n, sigma):
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


def launch_list(fn):
    """The library's launch record of fn(): the instantiation ids in launch order."""
    from dpc.render import _native as N

    L = N.lib()
    N.check(L.dpc_profile_enable(64), "dpc_profile_enable")
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.dpc_profile_disable()
    buf = ctypes.create_string_buffer(128)
    out = []
    for i in range(L.dpc_profile_count()):
        N.check(L.dpc_profile_get_id(i, buf, len(buf)), "dpc_profile_get_id")
        out.append(buf.value.decode())
    return out


def params(B, D, G, taps_z=0):
    from dpc.render import _native as N

    return N.DpcParams(B, 0, D, G, G, 0, taps_z, 2.0, 1.875, EPS, 10.0, 1, 0, None, None, None, None, None)


# ------------------------------------------------------------------------------------------------ 1. mask loss, C ABI
class MaskCase:
    def __init__(self, name, B, D, G, kz, s, f, weights, dloss, seed, kernel):
        self.name, self.B, self.D, self.G, self.kz, self.f, self.seed, self.kernel = name, B, D, G, kz, f, seed, kernel
        self.has_s, self.has_w, self.has_dloss = s, weights, dloss

    def __repr__(self):
        return self.name


# D = 32 / 64 / 128: the register instantiations; D = 24 and the 33-tap kernel: the generic kernels.  G = 24: 576 rays, the
# third ray tile is partly dead; G = 17: an odd width.  z radius 0 (no taps), 2, 15 (the largest compiled window), 16 (beyond).
MASK_CASES = [
    MaskCase("d32_g24_r2", 3, 32, 24, gauss(5, 0.9), True, 2, True, True, 1, "k_drcmask_bwd<32, 2>"),
    MaskCase("d64_g16_notaps", 2, 64, 16, None, False, 1, False, False, 2, "k_drcmask_bwd<64, 0>"),
    MaskCase("d128_g16_r15", 2, 128, 16, gauss(31, 6.0), True, 1, False, False, 15, "k_drcmask_bwd<128, 15>"),
    MaskCase("d24_g16_r2_dyn", 2, 24, 16, gauss(5, 0.9), True, 2, True, True, 4, "k_drcmask_bwd_dyn"),
    MaskCase("d32_g16_r16_dyn", 2, 32, 16, gauss(33, 7.0), True, 1, True, True, 5, "k_drcmask_bwd_dyn"),
    MaskCase("d32_g17_notaps_nos", 1, 32, 17, None, False, 1, False, False, 6, "k_drcmask_bwd<32, 0>"),
]


def mask_inputs(c):
    """Seeded fp32 inputs of a case (host tensors): a grid like the one the W and H passes leave (zeros and values up to a bit
    above 1; about four occupied voxels per ray whatever the depth -- a ray that surely ends in the grid has no gradient left),
    scales that push some s v beyond 1, masks like pooled ones (0, 1 and fractions), weights with one zero."""
    g = torch.Generator().manual_seed(9100 + c.seed)
    B, D, G, f = c.B, c.D, c.G, c.f
    grid = 0.02 + 1.08 * torch.rand(B, D, G, G, generator=g)
    dens = min(0.45, 4.0 / D)
    grid = grid * (torch.rand(B, D, G, G, generator=g) < dens) * (torch.rand(B, 1, G, G, generator=g) < 0.8)
    wide = c.kz is not None and len(c.kz) > 20   # a long kernel averages the sparse grid down: larger scales reach 1
    s = ((0.5 / dens if wide else 0.7) + (0.75 / dens if wide else 1.5) * torch.rand(B, generator=g)) if c.has_s else None
    masks = (torch.rand(B, f * G, f * G, generator=g) < 0.5).float()
    part = torch.rand(B, f * G, f * G, generator=g) < 0.3
    masks = torch.where(part, torch.rand(B, f * G, f * G, generator=g), masks)
    w = None
    if c.has_w:
        w = 0.5 + torch.rand(B, generator=g)
        w[0] = 0.0
    dloss = torch.tensor(0.5 + float(torch.rand(1, generator=g))) if c.has_dloss else None
    return grid.float(), s, masks.float(), w, dloss


_MASK_REF = {}


def mask_reference(c):
    """(loss, dgrid_wh, ds) of the oracle for the case's inputs, computed once and shared."""
    if c.name not in _MASK_REF:
        grid, s, masks, w, dloss = mask_inputs(c)
        margin = DR.clamp_margin(grid, s, c.kz, EPS)
        assert margin > MARGIN, "%s: a pre-clamp value lies %.2e from a clamp threshold" % (c.name, margin)
        if c.has_s:
            assert float(DR.DO.pre_clamp(grid, s, c.kz).max()) > 1.0, "no s v beyond 1"
        gd = grid.double().requires_grad_(True)
        sd = s.double().requires_grad_(True) if s is not None else None
        loss = DR.mask_loss(gd, sd, c.kz, masks, c.f, w, EPS)
        (loss * (dloss.double() if dloss is not None else 1.0)).backward()
        _MASK_REF[c.name] = (loss.detach(), gd.grad, sd.grad if sd is not None else None)
    return _MASK_REF[c.name]


@pytest.mark.parametrize("c", MASK_CASES, ids=repr)
def test_mask_abi_parity(c):
    """loss, dgrid_wh and ds of the two entry points; the instantiations they launch; a second forward + backward on the same
    workspace gives the same bits and leaves the tickets at zero."""
    from dpc.render import _native as N

    rloss, rdgrid, rds = mask_reference(c)
    grid, s, masks, w, dloss = (None if x is None else x.cuda().contiguous() for x in mask_inputs(c))
    B, D, G = c.B, c.D, c.G
    kz = None if c.kz is None else np.ascontiguousarray(c.kz, dtype=np.float32)
    P = params(B, D, G, 0 if kz is None else kz.size)
    ref, L = ctypes.byref(P), N.lib()
    kzp = None if kz is None else kz.ctypes.data_as(ctypes.c_void_p)
    tiles = torch.full((B, (G * G + 255) // 256), float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    dgrid = torch.full((B, D, G, G), float("nan"), device="cuda")     # overwritten: no pre-zeroing
    ds = torch.full((B,), float("nan"), device="cuda") if s is not None else None
    # the caller's part of the workspace contract: the tickets (first 4 * B bytes) zeroed once; the rest may hold anything
    ws = torch.full((max(L.dpc_drc_workspace_bytes(ref), 16),), 0xA5, dtype=torch.uint8, device="cuda")
    ws[:4 * B] = 0
    st = N.stream_ptr(torch.device("cuda"))

    def fwd():
        N.check(L.dpc_drc_loss_fwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(masks), c.f, N.ptr(w), N.ptr(tiles), N.ptr(loss), st),
                "dpc_drc_loss_fwd")

    def bwd():
        N.check(L.dpc_drc_loss_bwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(masks), c.f, N.ptr(w), N.ptr(dloss), N.ptr(dgrid),
                                   N.ptr(ds), N.ptr(ws), st), "dpc_drc_loss_bwd")

    lf, lb = launch_list(fwd), launch_list(bwd)
    assert lf == [c.kernel.replace("bwd", "fwd"), "k_tile_loss_finalize"] and lb == [c.kernel], (lf, lb)
    close(loss[0], rloss, what=c.name + " loss")
    close(dgrid, rdgrid, what=c.name + " dgrid_wh")
    if c.has_s:
        close(ds, rds, what=c.name + " ds")
    assert float(rdgrid.abs().max()) > 1e-3 and float(rloss) > 1.0
    first = (loss.clone(), dgrid.clone(), None if ds is None else ds.clone())
    for t in (loss, dgrid, ds):
        if t is not None:
            t.fill_(float("nan"))
    fwd()
    bwd()
    torch.cuda.synchronize()
    assert torch.equal(first[0], loss) and torch.equal(first[1], dgrid) and (ds is None or torch.equal(first[2], ds))
    assert int(ws[:4 * B].max()) == 0


def test_an_empty_batch_has_a_zero_loss():
    from dpc.render import _native as N

    L, st = N.lib(), N.stream_ptr(torch.device("cuda"))
    P = params(0, 32, 16)
    loss = torch.full((2,), float("nan"), device="cuda")
    assert L.dpc_drc_loss_fwd(ctypes.byref(P), None, None, None, None, 1, None, None, N.ptr(loss[:1]), st) == 0
    assert L.dpc_drc_rgb_loss_fwd(ctypes.byref(P), None, None, None, DIV_EPS, 0, None, 1, 0, None, None, N.ptr(loss[1:]), st) == 0
    assert L.dpc_drc_loss_bwd(ctypes.byref(P), None, None, None, None, 1, None, None, None, None, None, st) == 0
    assert L.dpc_drc_rgb_loss_bwd(ctypes.byref(P), None, None, None, DIV_EPS, 0, None, 1, 0, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert loss.tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ 2. colour loss, C ABI
class RgbCase:
    def __init__(self, name, D, G, f, divide, clip_after, planar, weights, dloss, seed, kernel):
        self.name, self.B, self.D, self.G, self.f, self.seed, self.kernel = name, 2, D, G, f, seed, kernel
        self.divide, self.clip_after, self.planar, self.has_w, self.has_dloss = divide, clip_after, planar, weights, dloss

    def __repr__(self):
        return self.name


RGB_CASES = [
    RgbCase("d32_g24_divide_planar_f2", 32, 24, 2, True, False, True, True, True, 1, "k_drcrgb_bwd<32>"),
    RgbCase("d64_g16_clip_after", 64, 16, 1, False, True, False, False, False, 2, "k_drcrgb_bwd<64>"),
    RgbCase("d24_g16_dyn", 24, 16, 1, True, False, False, True, False, 3, "k_drcrgb_bwd_dyn"),
    RgbCase("d128_g8_dyn", 128, 8, 2, False, True, True, False, True, 4, "k_drcrgb_bwd_dyn"),
]


def rgb_inputs(c):
    """Seeded fp32 host inputs: occupancies with many exact zeros and some values above 1 - eps, a colour grid with zeros and
    values up to 1.3 (the after-clip acts), occupancies to divide by, images (channel-last), weights with one zero."""
    g = torch.Generator().manual_seed(9200 + c.seed)
    B, D, G, f = c.B, c.D, c.G, c.f
    vox = torch.rand(B, D, G, G, generator=g)
    vox = vox * (torch.rand(B, D, G, G, generator=g) < 0.3) * (torch.rand(B, 1, G, G, generator=g) < 0.85)
    high = torch.rand(B, D, G, G, generator=g) < 0.01
    vox = torch.where(high, 1.0 - 0.4 * EPS * torch.rand(B, D, G, G, generator=g, dtype=torch.float64).float(), vox).float()
    C = 1.3 * torch.rand(B, 3, D, G, G, generator=g) * (torch.rand(B, 1, D, G, G, generator=g) < 0.6)
    div = (0.2 + 1.3 * torch.rand(B, D, G, G, generator=g)).float() if c.divide else None
    images = torch.rand(B, f * G, f * G, 3, generator=g)
    w = None
    if c.has_w:
        w = 0.5 + torch.rand(B, generator=g)
        w[0] = 0.0
    dloss = torch.tensor(0.5 + float(torch.rand(1, generator=g))) if c.has_dloss else None
    return vox, C.float(), div, images.float(), w, dloss


_RGB_REF = {}


def rgb_reference(c):
    """(loss, dvox, dC) of the oracle, computed once and shared."""
    if c.name not in _RGB_REF:
        vox, C, div, images, w, dloss = rgb_inputs(c)
        v = vox.double().reshape(-1)
        v = v[v != 0.0]
        drc = float(torch.stack([(v - EPS).abs().min(), (v - (1.0 - EPS)).abs().min()]).min())
        assert drc > MARGIN, "%s: an occupancy lies %.2e from eps or 1 - eps" % (c.name, drc)
        assert bool((vox > 1.0 - EPS).any()) and float((vox == 0).float().mean()) > 0.5
        clip = DR.clip_margin(C, div, DIV_EPS, c.clip_after)
        assert clip > MARGIN, "%s: a colour lies %.2e from a clip threshold" % (c.name, clip)
        if c.clip_after:
            assert int((C > 1.0).sum()) > 10, "the after-clip masks next to nothing"
        vd, Cd = vox.double().requires_grad_(True), C.double().requires_grad_(True)
        loss = DR.rgb_loss(vd, Cd, div, images, c.f, w, EPS, DIV_EPS, c.clip_after)
        (loss * (dloss.double() if dloss is not None else 1.0)).backward()
        _RGB_REF[c.name] = (loss.detach(), vd.grad, Cd.grad)
    return _RGB_REF[c.name]


@pytest.mark.parametrize("c", RGB_CASES, ids=repr)
def test_rgb_abi_parity(c):
    """loss, dvox and dC of the two entry points on a given colour grid; the instantiations they launch; the bits repeat."""
    from dpc.render import _native as N

    rloss, rdvox, rdC = rgb_reference(c)
    vox, C, div, images, w, dloss = rgb_inputs(c)
    if c.planar:
        images = images.permute(0, 3, 1, 2)
    vox, C, div, images, w, dloss = (None if x is None else x.cuda().contiguous() for x in (vox, C, div, images, w, dloss))
    B, D, G = c.B, c.D, c.G
    P = params(B, D, G)
    ref, L, st = ctypes.byref(P), N.lib(), N.stream_ptr(torch.device("cuda"))
    tiles = torch.full((B, (G * G + 255) // 256), float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    dvox = torch.full((B, D, G, G), float("nan"), device="cuda")      # overwritten: no pre-zeroing
    dC = torch.full((B, 3, D, G, G), float("nan"), device="cuda")

    def fwd():
        N.check(L.dpc_drc_rgb_loss_fwd(ref, N.ptr(vox), N.ptr(C), N.ptr(div), DIV_EPS, int(c.clip_after), N.ptr(images), c.f,
                                       int(c.planar), N.ptr(w), N.ptr(tiles), N.ptr(loss), st), "dpc_drc_rgb_loss_fwd")

    def bwd():
        N.check(L.dpc_drc_rgb_loss_bwd(ref, N.ptr(vox), N.ptr(C), N.ptr(div), DIV_EPS, int(c.clip_after), N.ptr(images), c.f,
                                       int(c.planar), N.ptr(w), N.ptr(dloss), N.ptr(dvox), N.ptr(dC), st), "dpc_drc_rgb_loss_bwd")

    lf, lb = launch_list(fwd), launch_list(bwd)
    assert lf == ["k_drcrgb_fwd", "k_tile_loss_finalize"] and lb == [c.kernel], (lf, lb)
    close(loss[0], rloss, what=c.name + " loss")
    close(dvox, rdvox, what=c.name + " dvox")
    close(dC, rdC, what=c.name + " dC")
    assert float(rdvox.abs().max()) > 1e-3 and float(rdC.abs().max()) > 1e-3 and float(rloss) > 1.0
    first = (loss.clone(), dvox.clone(), dC.clone())
    for t in (loss, dvox, dC):
        t.fill_(float("nan"))
    fwd()
    bwd()
    torch.cuda.synchronize()
    assert torch.equal(first[0], loss) and torch.equal(first[1], dvox) and torch.equal(first[2], dC)


# ------------------------------------------------------------------------------------------------ 3. dpc.render
@pytest.fixture(scope="module")
def exact_pose():
    O.EXACT_POSE_GRADIENT = True   # d(q) against the exact fp64 sum over the points, as tests/test_gpu_parity.py does
    yield O
    O.EXACT_POSE_GRADIENT = False


E2E = dict(B=2, N=200, G=32, taps=7, sigma=2.4, f=2, seed=3)


def e2e_cfg(**kw):
    return O.Cfg(vox_size=E2E["G"], pc_gauss_kernel_size=E2E["taps"], drc_logsum_clip_val=EPS,
                 pc_rgb_divide_by_occupancies=True, pc_rgb_divide_by_occupancies_epsilon=DIV_EPS, **kw)


def e2e_inputs():
    """Points constructed in the grid (cell uniform -- a third of them in ONE cell --, fraction in [1/4, 3/4] per axis) and
    taken back through the inverse camera, so that every trilinear weight is at least 1/64; with the wide Gaussian and scales in
    [0.8, 0.98] every non-zero occupancy then stays above eps (the construction of tests/test_rgb_loss_gpu.py)."""
    g = torch.Generator().manual_seed(8100 + E2E["seed"])
    B, G, N, f = E2E["B"], E2E["G"], E2E["N"], E2E["f"]
    cfg = e2e_cfg()
    q = torch.randn(B, 4, generator=g).float()
    s = (0.8 + 0.18 * torch.rand(B, 1, generator=g)).float()
    cell = torch.randint(0, G - 1, (B, N, 3), generator=g).double()
    nb = N // 3
    cell[:, :nb] = torch.randint(3, G - 4, (B, 1, 3), generator=g).double()
    zyx = (cell + 0.25 + 0.5 * torch.rand(B, N, 3, generator=g, dtype=torch.float64)) / (G - 1.0) - 0.5
    zyx[:, nb:nb + N // 20, 1] = 0.56 + 0.1 * torch.rand(B, N // 20, generator=g, dtype=torch.float64)
    zc = zyx[..., 0:1] + cfg.camera_distance
    moved = torch.cat([zyx[..., 0:1], zyx[..., 1:2] * zc / cfg.focal_length, zyx[..., 2:3] * zc / cfg.focal_length], 2)
    pc = O.quaternion_rotate(moved, q.double() * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64)).float()
    rgb = (0.05 + 0.9 * torch.rand(B, N, 3, generator=g)).float()
    masks = (torch.rand(B, 1, f * G, f * G, generator=g) < 0.5).float()
    images = torch.rand(B, f * G, f * G, 3, generator=g)
    w = 0.5 + torch.rand(B, generator=g)
    return pc, q, s, rgb, masks, images, w


_E2E = {}


def e2e_reference():
    """The oracle's chain (transform, splat, smoothing, scale, probabilities; colour splat, smoothing, division) with the two
    losses on its own tr_pc, voxels and probabilities; gradients to points, quaternions, scale and colours."""
    if not _E2E:
        pc, q, s, rgb, masks, images, w = e2e_inputs()
        cfg = e2e_cfg()
        kern = O.smoothing_kernel(cfg, E2E["sigma"])
        leaves = [x.clone().requires_grad_(True) for x in (pc, q, s, rgb)]
        ref = O.pointcloud_project_fast(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2])
        vox = ref["voxels"][..., 0]
        colour, drc = RO.clip_margin(cfg, ref["tr_pc"].detach(), rgb, vox.detach(), kern)
        assert colour > 1e-4 and drc > MARGIN, (colour, drc)
        raw, pre = ref["voxels_raw"].detach().reshape(-1), vox.detach().reshape(-1)
        assert float((raw[raw != 0] - 1.0).abs().min()) > 1e-4 and float((pre[pre != 0] - 1.0).abs().min()) > MARGIN
        assert int((pre != 0).sum()) > 5000
        p = ref["drc_probs"][..., 0].permute(1, 0, 2, 3)                        # [B,D+1,H,W], rows in image order
        mask = DR.mask_loss_of_probabilities(p, masks[:, 0], E2E["f"], w)
        proj, vrgb, half_sq = RO.rgb_loss(cfg, ref["tr_pc"], leaves[3], vox, kern, images, E2E["f"], w)
        drc_rgb = DR.rgb_loss_of_probabilities(p, vrgb, images, E2E["f"], w)
        grads = {}
        for name, loss in (("mask", mask), ("drc_rgb", drc_rgb), ("proj_rgb", half_sq)):
            got = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
            grads[name] = [None if x is None else x.detach() for x in got]
        _E2E.update(mask=mask.detach(), drc_rgb=drc_rgb.detach(), proj_rgb=half_sq.detach(), grads=grads)
    return _E2E


def e2e_device():
    import dpc.render as R

    pc, q, s, rgb, masks, images, w = e2e_inputs()
    cfg = e2e_cfg()
    kern = R.smoothing_kernel(cfg, E2E["sigma"])
    leaves = [dev(x, True) for x in (pc, q, s, rgb)]
    out = R.pointcloud_project_fast(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2])
    return R, cfg, kern, leaves, out, masks.cuda(), images.cuda(), w.cuda()


def test_drc_loss_end_to_end(exact_pose):
    ref = e2e_reference()
    R, cfg, kern, leaves, out, masks, images, w = e2e_device()
    loss = R.drc_loss(cfg, out, masks, w)
    close(loss, ref["mask"], what="e2e drc loss")
    assert torch.equal(loss, R.drc_loss(cfg, out, masks[:, 0], w)) and torch.equal(loss, R.drc_loss(cfg, out, masks.permute(0, 2, 3, 1), w))
    loss.backward()
    for name, x, r in zip(("points", "quaternions", "s"), leaves, ref["grads"]["mask"]):
        assert x.grad is not None and float(r.abs().max()) > 0, name
        close(x.grad, r, what="e2e drc d(%s)" % name)
    assert leaves[3].grad is None


def test_drc_rgb_loss_end_to_end(exact_pose):
    ref = e2e_reference()
    R, cfg, kern, leaves, out, masks, images, w = e2e_device()
    loss = R.drc_rgb_loss(cfg, out, leaves[3], images, kern, w)
    close(loss, ref["drc_rgb"], what="e2e drc_rgb loss")
    close(R.drc_rgb_loss(cfg, out, leaves[3], images.permute(0, 3, 1, 2).contiguous(), kern, w), ref["drc_rgb"], what="... planar images")
    loss.backward()
    for name, x, r in zip(("points", "quaternions", "s", "rgb"), leaves, ref["grads"]["drc_rgb"]):
        assert x.grad is not None and float(r.abs().max()) > 0, name
        close(x.grad, r, what="e2e drc_rgb d(%s)" % name)


def test_shared_grids_equal_the_sum_of_the_two_colour_losses(exact_pose):
    """proj_rgb_loss + drc_rgb_loss on one rgb_grids against the two computed separately: the colour splat's atomics leave
    the last bits open, nothing else differs (1e-5 rule); one splat and one set of smoothing passes instead of two."""
    from dpc.render import _native as N

    ref = e2e_reference()
    R, cfg, kern, leaves, out, masks, images, w = e2e_device()
    sep = R.proj_rgb_loss(cfg, out, leaves[3], images, kern, w) + R.drc_rgb_loss(cfg, out, leaves[3], images, kern, w)
    gsep = torch.autograd.grad(sep, leaves, retain_graph=True)
    launches = []

    def shared():
        grids = R.rgb_grids(cfg, out, leaves[3], kern)
        launches.append(R.proj_rgb_loss(cfg, out, leaves[3], images, kern, w, grids=grids)
                        + R.drc_rgb_loss(cfg, out, leaves[3], images, kern, w, grids=grids))

    ids = launch_list(shared)
    assert ids.count("k_rgb_splat") == 1, ids
    both = launches[0]
    gboth = torch.autograd.grad(both, leaves)
    close(both, sep.double(), what="shared grids: loss")
    close(both, ref["proj_rgb"] + ref["drc_rgb"], what="shared grids: loss vs oracle")
    for name, a, b, r1, r2 in zip(("points", "quaternions", "s", "rgb"), gboth, gsep, ref["grads"]["proj_rgb"], ref["grads"]["drc_rgb"]):
        close(a, b.double(), what="shared grids: d(%s)" % name)
        close(a, r1 + r2, what="shared grids: d(%s) vs oracle" % name)
    assert N.lib().dpc_abi_version() == 15


def test_staged_fallback_agrees_with_the_fused_path():
    R, cfg, kern, leaves, out, masks, images, w = e2e_device()
    fused = R.drc_loss(cfg, out, masks, w)
    gf = torch.autograd.grad(fused, leaves[:3])
    st = R._project_staged(cfg, R._geometry(cfg, kern), leaves[0], leaves[1], None, None, leaves[2], True)
    staged_out = R.ProjectionOutputs(st["proj"], lambda: st)
    assert staged_out._fused is None
    staged = R.drc_loss(cfg, staged_out, masks, w)
    gs = torch.autograd.grad(staged, leaves[:3])
    close(fused, staged.double(), what="fused vs staged drc loss")
    for name, a, b in zip(("points", "quaternions", "s"), gf, gs):
        close(a, b.double(), what="fused vs staged d(%s)" % name)


# ------------------------------------------------------------------------------------------------ 4. harness
def test_harness_drc_step():
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.step import TrainStep

    kw = dict(batch_size=1, step_size=2, vox_size=32, pc_num_points=256, pose_predictor_student=False, pc_point_dropout=1.0,
              pc_relative_sigma=1.0, pc_relative_sigma_end=1.0, input_shape=[64, 64, 3], pose_predict_num_candidates=1)
    cfg = chair_unsupervised(drc_weight=0.5, **kw)
    torch.manual_seed(0)
    step = TrainStep(cfg, torch.device("cuda"))
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 64, 64, generator=g).cuda()
    masks = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()
    total, out = step.loss(images, masks)
    want = cfg.proj_weight * out["proj_loss"].double() + 0.5 * out["drc_loss"].double()
    assert float((total - want).detach().abs()) <= 1e-12 * float(want.detach().abs()) and float(out["drc_loss"]) > 0
    before = [p.detach().clone() for p in step.nets.parameters()]
    step(images, masks)
    assert any(not torch.equal(a, b) for a, b in zip(before, step.nets.parameters()))
    assert all(torch.isfinite(p).all() for p in step.nets.parameters())
    with pytest.raises(NotImplementedError, match="drc_weight"):
        step.capture(images, masks)
    # pc_rgb: both colour terms on one set of grids
    cfg = chair_unsupervised(pc_rgb=True, proj_rgb_weight=1.0, drc_rgb_weight=0.25, drc_weight=0.5, **kw)
    torch.manual_seed(0)
    step = TrainStep(cfg, torch.device("cuda"))
    total, out = step.loss(images, masks)
    want = (out["proj_loss"].double() + 0.5 * out["drc_loss"].double() + out["rgb_loss"].double() + 0.25 * out["drc_rgb_loss"].double())
    assert float((total - want).detach().abs()) <= 1e-12 * float(want.detach().abs()) and float(out["drc_rgb_loss"]) > 0
    total.backward()
    grad = step.nets.decoder.rgb_raw_dec.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and bool(grad.any())
