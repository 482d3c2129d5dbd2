"""The fused expected-depth loss on the GPU (csrc/dpc_depth.hip) against the fp64 oracle of tests/depth_loss_oracle.py.

Every comparison uses the parity rule of tests/test_gpu_parity.py, max |device - reference| <= 1e-5 * max(1, max |reference|).
The gradients are discontinuous at the clamps, so every test asserts on the oracle that no pre-clamp value s v of its seeded
inputs lies within 1e-6 of eps, 1 - eps or 1 (exact zeros excepted); the seeds were checked on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import depth_loss_oracle as DO

pytestmark = pytest.mark.gpu

TOL = 1e-5


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
    print("%-40s max abs err %.3e  bound %.3e" % (what, err, tol * scale))
    assert err <= tol * scale, "%s: max abs err %.3e > %.1e * %.2f" % (what, err, tol, scale)

EPS, CAMERA, MAX_DEPTH, MAX_DATASET_DEPTH = 1e-5, 2.0, 7.5, 10.0
MARGIN = 1e-6


def gauss(n, sigma):
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


class Case:
    def __init__(self, name, B, D, G, kz, s, f, weights, ddepth, dloss, seed, kernel):
        self.name, self.B, self.D, self.G, self.kz, self.f, self.seed, self.kernel = name, B, D, G, kz, f, seed, kernel
        self.has_s, self.has_w, self.has_ddepth, self.has_dloss = s, weights, ddepth, dloss

    def __repr__(self):
        return self.name


# D = 32 / 64 / 128: the register instantiations; D = 24 and the 33-tap kernel: the generic kernels.  G = 24: 576 rays, the
# third ray tile is partly dead.  z radius 0 (no taps), 2, 15 (the largest compiled window), 16 (beyond it).
CASES = [
    Case("d32_g24_r2", 3, 32, 24, gauss(5, 0.9), True, 2, True, True, True, 1, "k_depth_bwd<32, 2>"),
    Case("d64_g16_notaps", 2, 64, 16, None, False, 1, False, False, False, 2, "k_depth_bwd<64, 0>"),
    Case("d128_g16_r15", 2, 128, 16, gauss(31, 6.0), True, 1, False, True, False, 15, "k_depth_bwd<128, 15>"),
    Case("d24_g16_r2_dyn", 2, 24, 16, gauss(5, 0.9), True, 2, True, True, True, 4, "k_depth_bwd_dyn"),
    Case("d32_g16_r16_dyn", 2, 32, 16, gauss(33, 7.0), True, 1, True, False, True, 5, "k_depth_bwd_dyn"),
    Case("d32_g17_notaps_nos", 1, 32, 17, None, False, 1, False, True, False, 6, "k_depth_bwd<32, 0>"),
]


def inputs(c):
    """Seeded fp32 inputs of a case (host tensors): a grid like the one the W and H passes leave (zeros and values up to a bit
    above 1), scales that push some s v beyond 1, depth maps with background pixels, weights with one zero."""
    g = torch.Generator().manual_seed(9000 + c.seed)
    B, D, G, f = c.B, c.D, c.G, c.f
    grid = 0.02 + 1.08 * torch.rand(B, D, G, G, generator=g)
    grid = grid * (torch.rand(B, D, G, G, generator=g) < 0.45) * (torch.rand(B, 1, G, G, generator=g) < 0.8)
    wide = c.kz is not None and len(c.kz) > 20   # a long kernel averages the sparse grid down: larger scales reach 1
    s = ((2.5 if wide else 0.7) + (3.0 if wide else 1.5) * torch.rand(B, generator=g)) if c.has_s else None
    depths = 1.5 + 1.5 * torch.rand(B, f * G, f * G, generator=g)
    depths[torch.rand(B, f * G, f * G, generator=g) < 0.3] = MAX_DATASET_DEPTH
    w = None
    if c.has_w:
        w = 0.5 + torch.rand(B, generator=g)
        w[0] = 0.0
    ddepth = torch.randn(B, G, G, generator=g) if c.has_ddepth else None
    dloss = torch.tensor(0.5 + float(torch.rand(1, generator=g))) if c.has_dloss else None
    return grid.float(), s, depths.float(), w, ddepth, dloss


_REF = {}


def reference(c):
    """(depth, loss, dgrid_wh, ds) of the oracle for the case's inputs, computed once and shared."""
    if c.name not in _REF:
        grid, s, depths, w, ddepth, dloss = inputs(c)
        margin = DO.clamp_margin(grid, s, c.kz, EPS)
        assert margin > MARGIN, "%s: a pre-clamp value lies %.2e from a clamp threshold" % (c.name, margin)
        if c.has_s:
            assert float(DO.pre_clamp(grid, s, c.kz).max()) > 1.0, "no s v beyond 1"
        gd = grid.double().requires_grad_(True)
        sd = s.double().requires_grad_(True) if s is not None else None
        depth, loss = DO.depth_loss(gd, sd, c.kz, depths, c.f, w, EPS, CAMERA, MAX_DEPTH, MAX_DATASET_DEPTH)
        total = loss * (dloss.double() if dloss is not None else 1.0)
        if ddepth is not None:
            total = total + (depth * ddepth.double()).sum()
        total.backward()
        _REF[c.name] = (depth.detach(), loss.detach(), gd.grad, sd.grad if sd is not None else None)
    return _REF[c.name]


def run_abi(c, profile=False, again=False):
    """The two C entry points on the case's inputs; returns device tensors (depth, loss, dgrid_wh, ds) and the launches."""
    from dpc.render import _native as N

    grid, s, depths, w, ddepth, dloss = (None if x is None else x.cuda().contiguous() for x in inputs(c))
    B, D, G = c.B, c.D, c.G
    kz = None if c.kz is None else np.ascontiguousarray(c.kz, dtype=np.float32)
    P = N.DpcParams(B, 0, D, G, G, 0, 0 if kz is None else kz.size, CAMERA, 1.875, EPS, MAX_DEPTH, 1, 0, None, None, None, None, None)
    ref, L = ctypes.byref(P), N.lib()
    kzp = None if kz is None else kz.ctypes.data_as(ctypes.c_void_p)
    ntile = (G * G + 255) // 256
    depth = torch.full((B, G, G), float("nan"), device="cuda")
    tiles = torch.full((B, ntile), float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    dgrid = torch.full((B, D, G, G), float("nan"), device="cuda")     # overwritten: no pre-zeroing
    ds = torch.full((B,), float("nan"), device="cuda") if s is not None else None
    # the caller's part of the workspace contract: the tickets (first 4 * B bytes) zeroed once; the rest may hold anything
    ws = torch.full((max(L.dpc_depth_workspace_bytes(ref), 16),), 0xA5, dtype=torch.uint8, device="cuda")
    ws[:4 * B] = 0
    st = N.stream_ptr(torch.device("cuda"))

    def fwd():
        N.check(L.dpc_depth_loss_fwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(depths), c.f, MAX_DATASET_DEPTH, N.ptr(w), N.ptr(depth),
                                     N.ptr(tiles), N.ptr(loss), st), "dpc_depth_loss_fwd")

    def bwd():
        N.check(L.dpc_depth_loss_bwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(depths), c.f, MAX_DATASET_DEPTH, N.ptr(w), N.ptr(dloss),
                                     N.ptr(ddepth), N.ptr(dgrid), N.ptr(ds), N.ptr(ws), st), "dpc_depth_loss_bwd")

    launches = None
    if profile:
        launches = (launch_list(fwd), launch_list(bwd))
    else:
        fwd()
        bwd()
    torch.cuda.synchronize()
    if again:   # a second backward on the SAME workspace: the kernel left the tickets at zero
        first = (dgrid.clone(), None if ds is None else ds.clone())
        dgrid.fill_(float("nan"))
        if ds is not None:
            ds.fill_(float("nan"))
        bwd()
        torch.cuda.synchronize()
        assert torch.equal(first[0], dgrid) and (ds is None or torch.equal(first[1], ds)), "second call on one workspace differs"
        assert int(ws[:4 * B].max()) == 0
    return depth, loss, dgrid, ds, launches


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


# ------------------------------------------------------------------------------------------------ 1. C ABI parity
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_abi_parity(c):
    rdepth, rloss, rdgrid, rds = reference(c)
    depth, loss, dgrid, ds, _ = run_abi(c)
    close(depth, rdepth, what=c.name + " depth")
    close(loss[0], rloss, what=c.name + " loss")
    close(dgrid, rdgrid, what=c.name + " dgrid_wh")
    if c.has_s:
        close(ds, rds, what=c.name + " ds")
    assert float(rdgrid.abs().max()) > 1e-3 and float(rdepth.min()) < 0.9 * MAX_DEPTH


def test_projection_only_and_incoming_gradient_alone():
    """gt_depth = NULL: the depth map alone, one launch; its backward takes ddepth alone."""
    from dpc.render import _native as N

    c = CASES[0]
    grid, s, _, _, ddepth, _ = (None if x is None else x.cuda().contiguous() for x in inputs(c))
    gd, sd = grid.double().cpu().requires_grad_(True), s.double().cpu().requires_grad_(True)
    rdepth = DO.depth_map(gd, sd, c.kz, EPS, CAMERA, MAX_DEPTH)
    (rdepth * ddepth.double().cpu()).sum().backward()
    P = N.DpcParams(c.B, 0, c.D, c.G, c.G, 0, c.kz.size, CAMERA, 1.875, EPS, MAX_DEPTH, 1, 0, None, None, None, None, None)
    ref, L, st = ctypes.byref(P), N.lib(), N.stream_ptr(torch.device("cuda"))
    kzp = c.kz.ctypes.data_as(ctypes.c_void_p)
    depth, dgrid, ds = torch.empty(c.B, c.G, c.G, device="cuda"), torch.empty_like(grid), torch.empty(c.B, device="cuda")
    ws = torch.zeros(L.dpc_depth_workspace_bytes(ref), dtype=torch.uint8, device="cuda")
    ids = launch_list(lambda: N.check(L.dpc_depth_loss_fwd(ref, N.ptr(grid), N.ptr(s), kzp, None, 1, 0.0, None, N.ptr(depth), None,
                                                          None, st), "dpc_depth_loss_fwd"))
    assert ids == ["k_depth_fwd<32, 2>"]
    N.check(L.dpc_depth_loss_bwd(ref, N.ptr(grid), N.ptr(s), kzp, None, 1, 0.0, None, None, N.ptr(ddepth), N.ptr(dgrid), N.ptr(ds),
                                 N.ptr(ws), st), "dpc_depth_loss_bwd")
    close(depth, rdepth, what="depth only")
    close(dgrid, gd.grad, what="dgrid_wh from ddepth")
    close(ds, sd.grad, what="ds from ddepth")


# ------------------------------------------------------------------------------------------------ 2. end to end
@pytest.fixture(scope="module")
def O():
    from oracle import dpc_oracle as O

    O.EXACT_POSE_GRADIENT = True   # d(q) against the exact fp64 sum over the points, as tests/test_gpu_parity.py does
    yield O
    O.EXACT_POSE_GRADIENT = False


E2E_SEED, E2E_SIGMA, E2E_TAPS = 31, 1.0, 3


def e2e_cfg(O):
    return O.Cfg(vox_size=32, pc_gauss_kernel_size=E2E_TAPS, max_depth=MAX_DEPTH, max_dataset_depth=MAX_DATASET_DEPTH)


def e2e_inputs(O, shared, B=4, N=500, G=32):
    """Poses, translations, focal lengths and scales of oracle.synth_inputs; the POINTS are constructed: drawn in the grid
    (cell uniform, fraction in [1/4, 3/4] per axis) and taken back through the inverse camera, so that every trilinear weight is
    at least 1/64 and, under the 3-tap Gaussian, every nonzero s v is above 1e-4 -- a Gaussian's tails or a point next to a cell
    face would put dozens of voxels within 1e-6 of eps at any seed.  shared: two point sets, each used by two clouds with the
    same camera, their own 400-point subsets (point_index) and their own scales."""
    cfg = e2e_cfg(O)
    _, q, s, _, t, f = O.synth_inputs(B, N, G, seed=E2E_SEED, with_t=True, with_f=True)
    g = torch.Generator().manual_seed(E2E_SEED)
    sets = B // 2 if shared else B
    if shared:
        q, t, f = (x[::2].repeat_interleave(2, dim=0).contiguous() for x in (q, t, f))
    qs, ts, fs = (x[::B // sets].double() for x in (q, t, f))
    cell = torch.randint(0, G - 1, (sets, N, 3), generator=g).double()
    zyx = (cell + 0.25 + 0.5 * torch.rand(sets, N, 3, generator=g, dtype=torch.float64)) / (G - 1) - 0.5
    zc = zyx[..., 0:1] + ts[:, None, 0:1] + cfg.camera_distance
    moved = torch.cat([zyx[..., 0:1] + ts[:, None, 0:1], zyx[..., 1:2] * zc / fs[:, None], zyx[..., 2:3] * zc / fs[:, None]], 2)
    pc = O.quaternion_rotate(moved - ts[:, None], qs * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64)).float()
    index = None
    if shared:
        index = torch.stack([torch.randperm(N, generator=g)[:400] for _ in range(B)])
    depths = 1.5 + 1.5 * torch.rand(B, 2 * G, 2 * G, 1, generator=g)
    depths[torch.rand(B, 2 * G, 2 * G, 1, generator=g) < 0.3] = MAX_DATASET_DEPTH
    w = 0.5 + torch.rand(B, generator=g)
    return pc, q, s, t, f, depths.float(), w.float(), index


def e2e_reference(O, shared):
    """Oracle loss, depth and gradients (points, quaternions, s, t, f) of the chain + depth loss."""
    cfg = e2e_cfg(O)
    pc, q, s, t, f, depths, w, index = e2e_inputs(O, shared)
    leaves = [x.clone().requires_grad_(True) for x in (pc, q, s, t, f)]
    pts = leaves[0]
    if shared:
        pts = pts.repeat_interleave(2, dim=0).gather(1, index.unsqueeze(-1).expand(-1, -1, 3))
    kern = O.smoothing_kernel(cfg, E2E_SIGMA)
    ref = O.pointcloud_project_fast(cfg, pts, leaves[1], leaves[3], None, kern, scaling_factor=leaves[2], focal_length=leaves[4])
    vox = O.smoothen_voxels3d(cfg, torch.clamp(ref["voxels_raw"].unsqueeze(1), 0.0, 1.0), kern).squeeze(1)
    x = (vox * leaves[2].double().reshape(-1, 1, 1, 1)).detach().reshape(-1)
    x = x[x != 0]
    margin = min(float((x - v).abs().min()) for v in (EPS, 1.0 - EPS, 1.0))
    assert margin > MARGIN, "a pre-clamp value lies %.2e from a clamp threshold" % margin
    assert x.numel() > 20000 and float(ref["voxels_raw"].detach().sum()) > 0.95 * pts.shape[0] * pts.shape[1]   # the points are in the grid
    loss = DO.loss_of_depth(ref["proj_depth"][..., 0], depths[..., 0], 2, w, cfg.max_depth, MAX_DATASET_DEPTH)
    loss.backward()
    return loss.detach(), ref["proj_depth"].detach(), [x.grad for x in leaves]


@pytest.mark.parametrize("shared", [False, True], ids=["own_points", "shared_sets_point_index"])
def test_end_to_end_gradients(O, shared):
    import dpc.render as R

    cfg = e2e_cfg(O)
    rloss, rdepth, rgrads = e2e_reference(O, shared)
    pc, q, s, t, f, depths, w, index = e2e_inputs(O, shared)
    leaves = [dev(x, True) for x in (pc, q, s, t, f)]
    out = R.pointcloud_project_fast(cfg, leaves[0], leaves[1], leaves[3], None, R.smoothing_kernel(cfg, E2E_SIGMA),
                                    scaling_factor=leaves[2], focal_length=leaves[4],
                                    point_index=None if index is None else index.cuda())
    loss = R.proj_depth_loss(cfg, out, depths.cuda(), w.cuda())
    close(loss, rloss, what="e2e loss")
    close(R.project_depth(out), rdepth, what="e2e depth")
    loss.backward()
    for name, x, r in zip(("points", "quaternions", "s", "t", "f"), leaves, rgrads):
        assert x.grad is not None and float(r.abs().max()) > 0, name
        close(x.grad, r, what="e2e d(%s)" % name)


# ------------------------------------------------------------------------------------------------ 3. the existing route
def test_agrees_with_the_lazy_proj_depth_route(O):
    import dpc.render as R

    cfg = e2e_cfg(O)
    pc, q, s, t, f, depths, w = (x.cuda() for x in e2e_inputs(O, False)[:7])
    out = R.pointcloud_project_fast(cfg, pc, q, t, None, R.smoothing_kernel(cfg, E2E_SIGMA), scaling_factor=s, focal_length=f)
    lazy = out["proj_depth"]
    close(R.project_depth(out), lazy.double(), 1e-6, "project_depth vs outputs['proj_depth']")   # two device paths
    g = DO.subsample(depths[..., 0].cpu(), 2, MAX_DEPTH, MAX_DATASET_DEPTH).cuda()
    sq = ((g - lazy[..., 0].double()) ** 2).sum((1, 2)) * w.double() ** 2
    close(R.proj_depth_loss(cfg, out, depths, w), 0.5 * sq.sum() / pc.shape[0], what="loss vs the lazy route")
    loss2, depth2 = R.proj_depth_loss(cfg, out, depths, w, return_depth=True)   # the map the loss launch writes on the way
    assert torch.equal(depth2, R.project_depth(out)) and torch.equal(loss2, R.proj_depth_loss(cfg, out, depths, w))
    again = R.pointcloud_project_fast(cfg, pc, q, t, None, R.smoothing_kernel(cfg, E2E_SIGMA), scaling_factor=s, focal_length=f)
    assert torch.equal(again["proj_depth"], lazy)   # the lazy entry keeps its route and its bits


# ------------------------------------------------------------------------------------------------ 4. determinism, launches
@pytest.mark.parametrize("c", [CASES[0], CASES[3]], ids=repr)
def test_bits_repeat_and_launch_counts(c):
    _, loss1, dgrid1, ds1, launches = run_abi(c, profile=True)
    _, loss2, dgrid2, ds2, _ = run_abi(c, again=True)
    assert torch.equal(loss1, loss2) and torch.equal(dgrid1, dgrid2) and torch.equal(ds1, ds2)
    assert torch.isfinite(dgrid1).all() and torch.isfinite(ds1).all()
    fwd, bwd = launches
    assert len(fwd) == 2 and fwd[1] == "k_tile_loss_finalize" and len(bwd) == 1, launches
    assert bwd[0] == c.kernel and fwd[0] == c.kernel.replace("bwd", "fwd"), launches


# ------------------------------------------------------------------------------------------------ 5. harness
def _harness(K, weight, **kw):
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.step import TrainStep

    cfg = chair_unsupervised(batch_size=1, step_size=2, vox_size=32, pc_num_points=256, pose_predict_num_candidates=K,
                             pose_predictor_student=K > 1, pc_point_dropout=1.0, pc_relative_sigma=1.0, pc_relative_sigma_end=1.0,
                             input_shape=[64, 64, 3], proj_depth_weight=weight, **kw)
    torch.manual_seed(0)
    return cfg, TrainStep(cfg, torch.device("cuda"))


def test_harness_depth_step():
    cfg, step = _harness(1, 0.5, max_depth=MAX_DEPTH, max_dataset_depth=MAX_DATASET_DEPTH)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 64, 64, generator=g).cuda()
    masks = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()
    depths = (1.5 + 1.5 * torch.rand(2, 64, 64, 1, generator=g)).cuda()
    grads = []
    for d in (depths, depths + 0.25):
        step.optimizer.zero_grad(set_to_none=True)
        total, out = step.loss(images, masks, depths=d)
        want = cfg.proj_weight * out["proj_loss"].double() + 0.5 * out["depth_loss"].double()
        assert float((total - want).detach().abs()) <= 1e-12 * float(want.detach().abs())
        assert out["projs_depth"].shape == (2, 32, 32, 1) and float(out["depth_loss"]) > 0
        assert not out["projs_depth"].requires_grad and float(out["projs_depth"].min()) >= 1.5 - 1e-4
        total.backward()
        grads.append(step.nets.decoder.pts_raw_fc.weight.grad.clone())
    assert torch.isfinite(grads[0]).all() and not torch.equal(grads[0], grads[1])   # only the depths changed
    step(images, masks, depths=depths)   # the whole step runs
    with pytest.raises(ValueError, match="depths"):
        step.loss(images, masks)
    with pytest.raises(NotImplementedError, match="proj_depth_weight"):
        step.capture(images, masks)
    cfg4, step4 = _harness(4, 0.5)
    with pytest.raises(NotImplementedError, match="pose_predict_num_candidates"):
        step4.loss(images, masks, depths=depths)
