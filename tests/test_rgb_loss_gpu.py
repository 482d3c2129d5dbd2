"""The colour node on the GPU (csrc/dpc_rgb_splat.hip, csrc/dpc_rgb.hip, dpc.render.project_rgb / proj_rgb_loss) against the fp64 oracle of
tests/rgb_oracle.py.

Every comparison uses the parity rule of tests/test_gpu_parity.py, max |device - reference| <= 1e-5 * max(1, max |reference|).
The gradients are discontinuous at the clips, so every case first asserts on the oracle that no non-zero colour value its
clips look at lies within 1e-4 of a threshold that can be crossed, and no non-zero occupancy within 1e-6 of eps or 1 - eps
(rgb_oracle.clip_margin); the seeds were checked on the CPU.

Two levels.  Node level: the colour node on hand-made transformed points and occupancies (a ProjectionOutputs holding them as
leaves) -- gradients to the colours, the transformed points and the occupancies.  End to end: pointcloud_project_fast +
proj_rgb_loss -- gradients to the points, the quaternions and the occupancy scale."""
import numpy as np
import pytest
import torch

import rgb_oracle as RO
from oracle import dpc_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
COLOUR_MARGIN, DRC_MARGIN = 1e-4, 1e-6
EPS = 1e-5


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


class Case:
    def __init__(self, name, B, D, G, N, taps, sigma, f=1, weights=False, extra=False, planar=False, seed=0, e2e_seed=0,
                 e2e_sigma=None, **options):
        self.name, self.B, self.D, self.G, self.N, self.taps, self.sigma, self.f = name, B, D, G, N, taps, sigma, f
        self.e2e_sigma = sigma if e2e_sigma is None else e2e_sigma
        self.weights, self.extra, self.planar, self.seed, self.e2e_seed, self.options = weights, extra, planar, seed, e2e_seed, options

    def __repr__(self):
        return self.name

    def cfg(self):
        return O.Cfg(vox_size=self.G, vox_size_z=-1 if self.D == self.G else self.D, pc_gauss_kernel_size=self.taps or 3,
                     drc_logsum_clip_val=EPS, pc_rgb_divide_by_occupancies_epsilon=0.01, **self.options)

    def kernel(self, mod, e2e=False):
        """The three separable kernels from `mod` (the oracle or dpc.render); None without taps."""
        return None if not self.taps else mod.smoothing_kernel(self.cfg(), self.e2e_sigma if e2e else self.sigma)


# G = 24: 576 rays, the third ray tile is partly dead; G = 17: an odd width; D = 64 against G = 16: a z kernel of 29 taps.
# extra: the loss scaled (dloss != 1) and a gradient arriving at the image and the colour grid of project_rgb as well.
CASES = [
    Case("d32_g24_f2_weights", 3, 32, 24, 400, 5, 1.6, f=2, weights=True, extra=True, seed=1, e2e_seed=1),
    Case("d24_g17_notaps", 2, 24, 17, 300, 0, 0.0, planar=True, seed=2, e2e_seed=2),
    Case("d64_g16_divide", 2, 64, 16, 300, 7, 2.4, seed=3, e2e_seed=3, pc_rgb_divide_by_occupancies=True),
    Case("d32_g16_clip_after", 2, 32, 16, 300, 7, 0.7, e2e_sigma=2.4, planar=True, seed=4, e2e_seed=4, pc_rgb_clip_after_conv=True),
    Case("d16_g16_stop_gradient", 2, 16, 16, 200, 5, 1.6, seed=5, e2e_seed=5, pc_rgb_stop_points_gradient=True),
]


def images_and_weights(c, g):
    images = torch.rand(c.B, c.f * c.G, c.f * c.G, 3, generator=g)
    w = None
    if c.weights:
        w = 0.5 + torch.rand(c.B, generator=g)
        w[0] = 0.0
    return images, w


def extras(c, g):
    """(dloss, gradient arriving at proj_rgb, gradient arriving at voxels_rgb) of a case with `extra`."""
    if not c.extra:
        return None
    return (0.5 + float(torch.rand(1, generator=g)), torch.randn(c.B, c.G, c.G, 3, generator=g),
            0.01 * torch.randn(c.B, c.D, c.G, c.G, 3, generator=g))


# ------------------------------------------------------------------------------------------------ node level
def node_inputs(c):
    """Seeded fp32 host inputs: transformed points (z,y,x) -- a third in a blob one cell wide, a twentieth outside the cube,
    one at exactly -1/2, one within 1e-6 below +1/2 --, colours in [0.05, 0.95], occupancies with many exact zeros and some
    values above 1 - eps, images, weights with one zero."""
    g = torch.Generator().manual_seed(7000 + c.seed)
    B, D, G, N = c.B, c.D, c.G, c.N
    tr = -0.45 + 0.9 * torch.rand(B, N, 3, generator=g)
    nb = N // 3
    span = torch.tensor([D - 1.0, G - 1.0, G - 1.0])
    cell = torch.stack([torch.randint(2, D - 3, (B, 1), generator=g), torch.randint(2, G - 3, (B, 1), generator=g),
                        torch.randint(2, G - 3, (B, 1), generator=g)], dim=-1).float()
    tr[:, :nb] = (cell + torch.rand(B, nb, 3, generator=g)) / span - 0.5
    out = nb + N // 20
    axis = torch.randint(0, 3, (B, out - nb), generator=g)
    far = (0.5 + 0.01 + 0.1 * torch.rand(B, out - nb, generator=g)) * (2.0 * torch.randint(0, 2, (B, out - nb), generator=g) - 1.0)
    tr[:, nb:out] = tr[:, nb:out].scatter(2, axis.unsqueeze(-1), far.unsqueeze(-1))
    tr[:, out, 0] = -0.5
    tr[:, out + 1, 2] = 0.5 - 5e-7
    tr = tr.float()
    rgb = (0.05 + 0.9 * torch.rand(B, N, 3, generator=g)).float()
    vox = torch.rand(B, D, G, G, generator=g)
    vox = vox * (torch.rand(B, D, G, G, generator=g) < 0.3) * (torch.rand(B, 1, G, G, generator=g) < 0.85)
    high = torch.rand(B, D, G, G, generator=g) < 0.01
    vox = torch.where(high, 1.0 - 0.4 * EPS * torch.rand(B, D, G, G, generator=g, dtype=torch.float64).float(), vox).float()
    images, w = images_and_weights(c, g)
    return tr, rgb, vox, images, w, extras(c, g)


def oracle_total(c, cfg, kern, tr, rgb, vox, images, w, extra):
    """(proj_rgb, voxels_rgb, loss, the scalar that is differentiated) of the oracle."""
    proj, vrgb, loss = RO.rgb_loss(cfg, tr, rgb, vox, kern, images, c.f, w)
    total = loss
    if extra is not None:
        total = extra[0] * loss + (proj * extra[1].double()).sum() + (vrgb * extra[2].double()).sum()
    return proj, vrgb, loss, total


def assert_margins(c, cfg, kern, tr, rgb, vox, clip_acts=True):
    colour, drc = RO.clip_margin(cfg, tr, rgb, vox, kern)
    assert colour > COLOUR_MARGIN, "%s: a colour value lies %.2e from a clip threshold" % (c.name, colour)
    assert drc > DRC_MARGIN, "%s: an occupancy lies %.2e from eps or 1 - eps" % (c.name, drc)
    parts = {}
    with torch.no_grad():
        RO.colour_grid(cfg, tr, rgb, kern, parts)
    assert float(parts["raw"].max()) > 1.0, "the blob does not push a raw colour above 1"
    acted = parts["after_clip"] if cfg.pc_rgb_clip_after_conv else parts["pre_clip"]
    assert not clip_acts or int((acted > 1.0).sum()) >= 3, "the clip masks next to nothing"


_NODE = {}


def node_reference(c):
    """Oracle results of the node-level case, computed once and shared."""
    if c.name not in _NODE:
        tr, rgb, vox, images, w, extra = node_inputs(c)
        cfg, kern = c.cfg(), c.kernel(O)
        assert_margins(c, cfg, kern, tr, rgb, vox)
        assert bool((vox > 1.0 - EPS).any()) and float((vox == 0).float().mean()) > 0.5
        inside = ((tr >= -0.5) & (tr <= 0.5)).all(-1)
        assert int((~inside).sum()) >= c.B and bool((tr == -0.5).any()) and bool(((tr > 0.5 - 1e-6) & (tr < 0.5)).any())
        leaves = [x.double().requires_grad_(True) for x in (tr, rgb, vox)]
        proj, vrgb, loss, total = oracle_total(c, cfg, kern, *leaves, images, w, extra)
        total.backward()
        _NODE[c.name] = dict(proj=proj.detach(), vrgb=vrgb.detach(), loss=loss.detach(), inside=inside,
                             grads=[x.grad for x in leaves])
    return _NODE[c.name]


def fake_outputs(tr, vox):
    """A projection's outputs holding hand-made transformed points and occupancies."""
    import dpc.render as R

    return R.ProjectionOutputs(torch.zeros(vox.shape[0], vox.shape[2], vox.shape[3], 1, device=vox.device),
                               lambda: {"tr_pc": tr, "voxels": vox.unsqueeze(-1)})


def device_images(c, images):
    return (images.permute(0, 3, 1, 2).contiguous() if c.planar else images).cuda()


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_node_parity(c):
    import dpc.render as R

    ref = node_reference(c)
    tr, rgb, vox, images, w, extra = node_inputs(c)
    cfg, kern = c.cfg(), c.kernel(R)
    leaves = [dev(x, True) for x in (tr, rgb, vox)]
    out = fake_outputs(leaves[0], leaves[2])
    wd = None if w is None else w.cuda()
    loss, proj = R.proj_rgb_loss(cfg, out, leaves[1], device_images(c, images), kern, wd, return_rgb=True)
    maps = R.project_rgb(cfg, out, leaves[1], kern)
    close(loss, ref["loss"], what=c.name + " loss")
    close(proj, ref["proj"], what=c.name + " proj_rgb (loss launch)")
    close(maps["proj_rgb"], ref["proj"], what=c.name + " proj_rgb")
    close(maps["voxels_rgb"], ref["vrgb"], what=c.name + " voxels_rgb")
    assert maps["proj_rgb"].shape == (c.B, c.G, c.G, 3) and maps["voxels_rgb"].shape == (c.B, c.D, c.G, c.G, 3)
    assert not proj.requires_grad and maps["proj_rgb"].requires_grad
    total = loss
    if extra is not None:
        total = extra[0] * loss + (maps["proj_rgb"] * extra[1].cuda()).sum() + (maps["voxels_rgb"] * extra[2].cuda()).sum()
    total.backward()
    dtr, drgb, dvox = (x.grad for x in leaves)
    rtr, rrgb, rvox = ref["grads"]
    close(drgb, rrgb, what=c.name + " d(rgb)")
    close(dvox, rvox, what=c.name + " d(vox)")
    assert float(rrgb.abs().max()) > 1e-4 and float(rvox.abs().max()) > 1e-4
    outside = ~ref["inside"].cuda()
    assert not drgb[outside].any(), "a point outside the cube got a colour gradient"
    if cfg.pc_rgb_stop_points_gradient:
        assert rtr is None or not rtr.any()
        assert dtr is None or not dtr.any(), "pc_rgb_stop_points_gradient: the colour node sent a gradient to the points"
    else:
        close(dtr, rtr, what=c.name + " d(tr)")
        assert float(rtr.abs().max()) > 1e-3 and not dtr[outside].any()


def test_loss_bits_repeat_on_one_colour_grid():
    """Two runs of the loss entry point on the same grids: bit-equal loss and image (fixed-order tile sums, no atomics)."""
    import dpc.render as R
    from dpc.render._ops import RgbLoss, RgbSplat

    c = CASES[0]
    tr, rgb, vox, images, w, _ = node_inputs(c)
    geom = R._geometry(c.cfg(), None)
    C = torch.clamp(RgbSplat.apply(tr.cuda(), rgb.cuda(), geom, False), 0.0, 1.0)
    runs = [RgbLoss.apply(vox.cuda(), C, None, images.cuda(), c.f, False, w.cuda(), geom, 0.01, False) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][0]) and float(runs[0][0]) > 0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def exact_pose():
    O.EXACT_POSE_GRADIENT = True   # d(q) against the exact fp64 sum over the points, as tests/test_gpu_parity.py does
    yield O
    O.EXACT_POSE_GRADIENT = False


def e2e_inputs(c):
    """Points constructed in the grid (cell uniform -- a third of them in ONE cell --, fraction in [1/4, 3/4] per axis) and
    taken back through the inverse camera, so that every trilinear weight is at least 1/64; with the wide Gaussians of the
    cases and scales in [0.8, 0.98] every non-zero occupancy then stays above eps (tests/test_depth_loss_gpu.py has the
    reasoning).  A twentieth of the points are pushed out of the cube."""
    g = torch.Generator().manual_seed(8000 + c.e2e_seed)
    B, D, G, N = c.B, c.D, c.G, c.N
    cfg = c.cfg()
    q = torch.randn(B, 4, generator=g).float()
    s = (0.8 + 0.18 * torch.rand(B, 1, generator=g)).float()
    cell = torch.stack([torch.randint(0, D - 1, (B, N), generator=g), torch.randint(0, G - 1, (B, N), generator=g),
                        torch.randint(0, G - 1, (B, N), generator=g)], dim=-1).double()
    nb = N // 3
    cell[:, :nb] = torch.stack([torch.randint(3, D - 4, (B, 1), generator=g), torch.randint(3, G - 4, (B, 1), generator=g),
                                torch.randint(3, G - 4, (B, 1), generator=g)], dim=-1).double()
    span = torch.tensor([D - 1.0, G - 1.0, G - 1.0], dtype=torch.float64)
    zyx = (cell + 0.25 + 0.5 * torch.rand(B, N, 3, generator=g, dtype=torch.float64)) / span - 0.5
    zyx[:, nb:nb + N // 20, 1] = 0.56 + 0.1 * torch.rand(B, N // 20, generator=g, dtype=torch.float64)
    zc = zyx[..., 0:1] + cfg.camera_distance
    moved = torch.cat([zyx[..., 0:1], zyx[..., 1:2] * zc / cfg.focal_length, zyx[..., 2:3] * zc / cfg.focal_length], 2)
    pc = O.quaternion_rotate(moved, q.double() * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=torch.float64)).float()
    rgb = (0.05 + 0.9 * torch.rand(B, N, 3, generator=g)).float()
    images, w = images_and_weights(c, g)
    return pc, q, s, rgb, images, w


_E2E = {}


def e2e_reference(c):
    if c.name not in _E2E:
        pc, q, s, rgb, images, w = e2e_inputs(c)
        cfg, kern = c.cfg(), c.kernel(O, e2e=True)
        leaves = [x.clone().requires_grad_(True) for x in (pc, q, s, rgb)]
        ref = O.pointcloud_project_fast(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2])
        vox = ref["voxels"][..., 0]
        # the wide Gaussian that keeps the occupancies off eps spreads the blob below 1: the after-clip acts at node level only
        assert_margins(c, cfg, kern, ref["tr_pc"].detach(), rgb, vox.detach(), clip_acts=not cfg.pc_rgb_clip_after_conv)
        # the occupancy chain's own clips: raw splat against 1, scaled grid against 1
        raw = ref["voxels_raw"].detach().reshape(-1)
        pre = vox.detach().reshape(-1)
        assert float((raw[raw != 0] - 1.0).abs().min()) > COLOUR_MARGIN and float((pre[pre != 0] - 1.0).abs().min()) > DRC_MARGIN
        proj, vrgb, loss = RO.rgb_loss(cfg, ref["tr_pc"], leaves[3], vox, kern, images, c.f, w)
        loss.backward()
        _E2E[c.name] = dict(proj=proj.detach(), loss=loss.detach(), grads=[x.grad for x in leaves])
    return _E2E[c.name]


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_end_to_end_gradients(exact_pose, c):
    import dpc.render as R

    ref = e2e_reference(c)
    pc, q, s, rgb, images, w = e2e_inputs(c)
    cfg, kern = c.cfg(), c.kernel(R, e2e=True)
    leaves = [dev(x, True) for x in (pc, q, s, rgb)]
    out = R.pointcloud_project_fast(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2])
    loss, proj = R.proj_rgb_loss(cfg, out, leaves[3], device_images(c, images), kern, None if w is None else w.cuda(),
                                 return_rgb=True)
    assert out["voxels_rgb"] is None and out["proj_rgb"] is None   # the projection's own dict keeps its empty colour entries
    close(loss, ref["loss"], what=c.name + " e2e loss")
    close(proj, ref["proj"], what=c.name + " e2e proj_rgb")
    loss.backward()
    for name, x, r in zip(("points", "quaternions", "s", "rgb"), leaves, ref["grads"]):
        assert x.grad is not None and float(r.abs().max()) > 0, name
        close(x.grad, r, what=c.name + " e2e d(%s)" % name)


# ------------------------------------------------------------------------------------------------ harness
def test_harness_colour_step():
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.step import TrainStep

    kw = dict(batch_size=1, step_size=2, vox_size=16, pc_num_points=200, pose_predictor_student=False, pc_point_dropout=1.0,
              pc_relative_sigma=1.0, pc_relative_sigma_end=1.0, input_shape=[64, 64, 3], pc_rgb=True, proj_rgb_weight=1.0)
    cfg = chair_unsupervised(pose_predict_num_candidates=1, **kw)
    torch.manual_seed(0)
    step = TrainStep(cfg, torch.device("cuda"))
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 64, 64, generator=g).cuda()
    masks = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()
    total, out = step.loss(images, masks)
    want = cfg.proj_weight * out["proj_loss"].double() + cfg.proj_rgb_weight * out["rgb_loss"].double()
    assert torch.isfinite(total) and float(out["rgb_loss"].detach()) > 0
    assert float((total - want).detach().abs()) <= 1e-6 * float(want.detach().abs())
    assert out["projs_rgb"].shape == (2, 16, 16, 3) and not out["projs_rgb"].requires_grad
    assert out["all_rgb"].shape == (2, 200, 3)
    total.backward()
    grad = step.nets.decoder.rgb_raw_dec.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and bool(grad.any())
    step(images, masks)   # the whole step runs
    with pytest.raises(NotImplementedError, match="proj_rgb_weight"):
        step.capture(images, masks)
    step4 = TrainStep(chair_unsupervised(pose_predict_num_candidates=4, **kw), torch.device("cuda"))
    with pytest.raises(NotImplementedError, match="pose_predict_num_candidates"):
        step4.loss(images, masks)
