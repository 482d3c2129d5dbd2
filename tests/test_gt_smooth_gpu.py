"""The ground-truth node on the GPU (csrc/dpc_gt_smooth.hip, dpc.render.smooth_gt) against the fp64 oracle of
tests/gt_smooth_oracle.py, the losses on prepared ground truth against their own oracles fed the oracle-smoothed target, and
the training step with cfg.pc_gauss_filter_gt, eager and captured.

Every comparison uses the parity rule of tests/test_gpu_parity.py, max |device - reference| <= 1e-5 * max(1, max |reference|),
except where bits are demanded.  The shapes are the smallest at which each part can break: both borders inside every window,
odd and non-square planes, more than one tile along each axis and tiles cut by the plane's edge (the tile is 16 rows x 64
columns), a radius of almost the side, and the largest plane the entry accepts."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gt_smooth_oracle as GO

pytestmark = pytest.mark.gpu

TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = {"mean": 0, "sample": 1}


def close(a, b, tol=TOL, what=""):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    a = a.reshape(b.shape) if a.size == b.size else a
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what + ": non-finite values"
    err = float(np.abs(a - b).max()) if a.size else 0.0
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    print("%-48s max abs err %.3e  bound %.3e" % (what, err, tol * scale))
    assert err <= tol * scale, "%s: max abs err %.3e > %.1e * %.2f" % (what, err, tol, scale)


def taps32(n, sigma):
    import dpc.render as R

    return R.gauss_kernel_1d(n, sigma).numpy()


def abi(gt, C, planar, H, W, mode, taps=None, dev_taps=None, ntaps=None, remap=(0.0, 0.0)):
    """dpc_gt_smooth on a device tensor gt (either layout) -> [S,H,W,C] device tensor."""
    from dpc.render import _native as N

    S = gt.shape[0]
    Hs, Ws = (gt.shape[2], gt.shape[3]) if planar else (gt.shape[1], gt.shape[2])
    gt = gt.contiguous()
    out = torch.full((S, H, W, C), float("nan"), dtype=torch.float32, device="cuda")
    host = None
    if taps is not None:
        host = np.ascontiguousarray(taps, dtype=np.float32)
        ntaps = host.size
    rc = N.lib().dpc_gt_smooth(N.ptr(gt), S, C, Hs, Ws, int(planar), H, W, MODES[mode], remap[0], remap[1],
                               None if host is None else host.ctypes.data_as(ctypes.c_void_p), N.ptr(dev_taps), ntaps, N.ptr(out),
                               N.stream_ptr(gt.device))
    N.check(rc, "dpc_gt_smooth")
    torch.cuda.synchronize()
    return out


class Case:
    def __init__(self, name, kind, S, H, W, f, n, sigma, seed, remap=(0.0, 0.0)):
        self.name, self.kind, self.S, self.H, self.W, self.f, self.n, self.sigma, self.seed, self.remap = name, kind, S, H, W, f, n, sigma, seed, remap
        self.C = 3 if kind == "images" else 1
        self.mode = "mean" if kind == "masks" else "sample"

    def __repr__(self):
        return self.name


CASES = [
    Case("m8_from16_11taps", "masks", 2, 8, 8, 2, 11, 1.0, 1),             # every pixel sees both borders
    Case("i6x10_5taps", "images", 2, 6, 10, 1, 5, 0.8, 2),                 # non-square, odd, three channels
    Case("m64_from128_21taps", "masks", 4, 64, 64, 2, 21, 3.0, 3),         # the experiments' shape: four row tiles
    Case("d24_from48_remap_7taps", "depths", 2, 24, 24, 2, 7, 1.5, 4, (10.0, 5.0)),
    Case("m32_63taps", "masks", 1, 32, 32, 1, 63, 8.0, 5),                 # the radius is almost the side
    Case("m37x70_11taps", "masks", 1, 37, 70, 1, 11, 1.7, 6),              # 37 = 2 * 16 + 5 rows, 70 = 64 + 6 columns
    Case("i199_from398_21taps", "images", 1, 199, 199, 2, 21, 4.0, 7),     # the largest projection
    Case("m1024_5taps", "masks", 1, 1024, 1024, 1, 5, 1.0, 8),             # the largest plane the entry accepts
]
_REF = {}


def inputs(c):
    """Seeded fp32 ground truth of a case, channel-last [S,Hs,Ws,C] (host)."""
    rng = np.random.RandomState(2700 + c.seed)
    shape = (c.S, c.f * c.H, c.f * c.W, c.C)
    if c.kind == "masks":
        gt = (rng.rand(*shape) < 0.45).astype(np.float32)
    elif c.kind == "images":
        gt = rng.rand(*shape).astype(np.float32)
    else:
        gt = (1.5 + 1.5 * rng.rand(*shape)).astype(np.float32)
        gt[rng.rand(*shape) < 0.35] = c.remap[0]     # background next to foreground all over the plane
        gt[0, 0, 0, 0], gt[0, 0, c.f, 0] = c.remap[0], 2.25
    return gt


def reference(c):
    if c.name not in _REF:
        ref = GO.smooth_gt(inputs(c), c.C, False, c.f, c.mode, taps32(c.n, c.sigma), *c.remap)
        ref.setflags(write=False)
        _REF[c.name] = ref
    return _REF[c.name]


def cfg_of(c, **kw):
    from dpc.harness.config import chair_unsupervised

    return chair_unsupervised(vox_size=c.H, pc_gauss_kernel_size=c.n, max_depth=5.0, max_dataset_depth=10.0, **kw)


# ------------------------------------------------------------------------------------------------ 1. the node
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_node_against_the_oracle(c):
    import dpc.render as R

    gt = torch.from_numpy(inputs(c)).cuda()
    planar = gt.permute(0, 3, 1, 2).contiguous()
    ref = reference(c)
    got = abi(gt, c.C, False, c.H, c.W, c.mode, taps32(c.n, c.sigma), remap=c.remap)
    close(got, ref, what=c.name + " C ABI")
    assert torch.equal(abi(planar, c.C, True, c.H, c.W, c.mode, taps32(c.n, c.sigma), remap=c.remap), got), "planar vs channel-last"
    assert torch.equal(abi(gt, c.C, False, c.H, c.W, c.mode, taps32(c.n, c.sigma), remap=c.remap), got), "a second run"
    via = R.smooth_gt(cfg_of(c), gt if c.kind == "images" else planar, (c.H, c.W), c.kind, sigma_rel=c.sigma)
    assert via.dtype == torch.float32 and not via.requires_grad and torch.equal(via, got), "smooth_gt vs the C ABI"
    if c.kind == "depths":     # the remap ran, and before the resize: the smoothed map never exceeds max_depth
        assert float(got.max()) <= 5.0 + 1e-5 and float(ref.max()) > 4.0


@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("C", [1, 3])
def test_one_tap_of_one_returns_the_resized_bits(mode, C):
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(2, C, 3 * 20, 3 * 70, generator=g).cuda()
    got = abi(gt, C, True, 20, 70, mode, np.ones(1, dtype=np.float32))
    ref = F.avg_pool2d(gt, 3) if mode == "mean" else gt[:, :, ::3, ::3]
    assert torch.equal(got, ref.permute(0, 2, 3, 1))
    # an identity kernel of any length: finite values times exactly 1 and 0
    ident = np.zeros(21, dtype=np.float32)
    ident[10] = 1.0
    assert torch.equal(abi(gt, C, True, 20, 70, mode, ident), got)


def test_device_taps_equal_host_taps():
    import dpc.render as R

    c = CASES[2]
    gt = torch.from_numpy(inputs(c)).cuda().permute(0, 3, 1, 2).contiguous()
    k = taps32(c.n, c.sigma)
    host = abi(gt, 1, True, c.H, c.W, "mean", k)
    sched = R.DeviceSchedule(torch.device("cuda"), k, k)
    assert torch.equal(abi(gt, 1, True, c.H, c.W, "mean", dev_taps=sched.taps_xy, ntaps=c.n), host)
    assert torch.equal(R.smooth_gt(cfg_of(c), gt, c.H, "masks", schedule=sched), host)
    assert torch.equal(R.smooth_gt(cfg_of(c), gt, c.H, "masks", kernel=R.smoothing_kernel(cfg_of(c), c.sigma)), host)
    # the values are read when the node runs: new taps in the same buffer, new output
    taps = R.DeviceTaps(torch.device("cuda"), k)
    assert torch.equal(R.smooth_gt(cfg_of(c), gt, c.H, "masks", schedule=taps), host)
    taps.update(taps32(c.n, 1.1))
    close(R.smooth_gt(cfg_of(c), gt, c.H, "masks", schedule=taps), GO.smooth_gt(inputs(c), 1, False, 2, "mean", taps32(c.n, 1.1)),
          what="device taps after an update")


def test_switch_off_and_gauss_smoothen_image():
    import dpc.render as R

    c = CASES[0]
    gt = torch.from_numpy(inputs(c)).cuda().permute(0, 3, 1, 2).contiguous()
    off = cfg_of(c, pc_gauss_filter_gt_switch_off=True)
    assert torch.equal(R.smooth_gt(off, gt, 8, "masks", sigma_rel=0.99), F.avg_pool2d(gt, 2).permute(0, 2, 3, 1))
    close(R.smooth_gt(off, gt, 8, "masks", sigma_rel=1.0), reference(c), what="switch-off at sigma_rel = 1.0: smoothed")
    close(R.smooth_gt(cfg_of(c), gt, 8, "masks", sigma_rel=0.99), GO.smooth_gt(inputs(c), 1, False, 2, "mean", taps32(11, 0.99)),
          what="without the switch: smoothed below 1")
    img = torch.rand(2, 8, 8, 3, generator=torch.Generator().manual_seed(12))
    close(R.gauss_smoothen_image(cfg_of(c), img.cuda(), 1.2), GO.smooth_gt(img.numpy(), 3, False, 1, "sample", taps32(11, 1.2)),
          what="gauss_smoothen_image [2,8,8,3]")


# ------------------------------------------------------------------------------------------------ 2. the losses
_E2E = {}


def e2e():
    """The projection of tests/test_drc_loss_gpu.py's end-to-end case (its seeded points keep every clamp at a distance) with
    ground truth smoothed by the oracle: reference losses and gradients, computed once."""
    import depth_loss_oracle as DO
    import drc_loss_oracle as DR
    import rgb_oracle as RO
    import test_drc_loss_gpu as TD
    from oracle import dpc_oracle as O

    if not _E2E:
        pc, q, s, rgb, masks, images, w = TD.e2e_inputs()
        G, f, sigma = TD.E2E["G"], TD.E2E["f"], TD.E2E["sigma"]
        cfg = TD.e2e_cfg()
        depths = 1.5 + 1.5 * torch.rand(2, f * G, f * G, 1, generator=torch.Generator().manual_seed(5))
        k = taps32(TD.E2E["taps"], sigma)
        gm = torch.from_numpy(GO.smooth_gt(masks.numpy(), 1, True, f, "mean", k))
        gi = torch.from_numpy(GO.smooth_gt(images.numpy(), 3, False, f, "sample", k))
        gd = torch.from_numpy(GO.smooth_gt(depths.numpy(), 1, False, f, "sample", k))
        O.EXACT_POSE_GRADIENT = True
        try:
            kern = O.smoothing_kernel(cfg, sigma)
            leaves = [x.clone().requires_grad_(True) for x in (pc, q, s, rgb)]
            ref = O.pointcloud_project_fast(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2])
            vox = ref["voxels"][..., 0]
            p = ref["drc_probs"][..., 0].permute(1, 0, 2, 3)
            losses = {"drc": DR.mask_loss_of_probabilities(p, gm[..., 0], 1, w),
                      "depth": DO.loss_of_depth(ref["proj_depth"][..., 0], gd[..., 0], 1, w),
                      "rgb": RO.rgb_loss(cfg, ref["tr_pc"], leaves[3], vox, kern, gi, 1, w)[2],
                      "proj": O.proj_loss_pose_candidates(gm[:1], ref["proj"], 2)[0]}
            winner = O.proj_loss_pose_candidates(gm[:1], ref["proj"], 2)[1]
            grads = {}
            for name, loss in losses.items():
                got = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
                grads[name] = [None if x is None else x.detach() for x in got]
        finally:
            O.EXACT_POSE_GRADIENT = False
        _E2E.update(losses={n: v.detach() for n, v in losses.items()}, grads=grads, winner=winner, depths=depths)
    return _E2E


def e2e_device(**keys):
    import dpc.render as R
    import test_drc_loss_gpu as TD

    pc, q, s, rgb, masks, images, w = TD.e2e_inputs()
    cfg = TD.e2e_cfg(**keys)
    kern = R.smoothing_kernel(cfg, TD.E2E["sigma"])
    leaves = [x.cuda().float().requires_grad_(True) for x in (pc, q, s, rgb)]
    return R, TD, cfg, kern, leaves, masks.cuda(), images.cuda(), w.cuda()


def check_grads(leaves, ref, what, names=("points", "quaternions", "s", "rgb")):
    for name, x, r in zip(names, leaves, ref):
        if r is None:
            assert x.grad is None, name
            continue
        assert x.grad is not None and float(r.abs().max()) > 0, name
        close(x.grad, r, what="%s d(%s)" % (what, name))


@pytest.mark.parametrize("which", ["drc", "depth", "rgb"])
def test_losses_on_prepared_ground_truth(which):
    ref = e2e()
    R, TD, cfg, kern, leaves, masks, images, w = e2e_device(pc_gauss_filter_gt=True, pc_gauss_filter_gt_rgb=True)
    G, sigma = TD.E2E["G"], TD.E2E["sigma"]
    out = R.pointcloud_project_fast(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2])
    if which == "drc":
        loss = R.drc_loss(cfg, out, R.smooth_gt(cfg, masks, G, "masks", sigma_rel=sigma), w, gt_prepared=True)
    elif which == "depth":
        loss = R.proj_depth_loss(cfg, out, R.smooth_gt(cfg, ref["depths"].cuda(), G, "depths", sigma_rel=sigma), w, gt_prepared=True)
    else:
        loss = R.proj_rgb_loss(cfg, out, leaves[3], R.smooth_gt(cfg, images, G, "images", kernel=kern), kern, w, gt_prepared=True)
    close(loss, ref["losses"][which], what=which + " loss on prepared ground truth")
    loss.backward()
    check_grads(leaves, ref["grads"][which], which)


def test_project_loss_with_two_candidates_on_prepared_masks():
    ref = e2e()
    R, TD, cfg, kern, leaves, masks, images, w = e2e_device(pc_gauss_filter_gt=True)
    gm = R.smooth_gt(cfg, masks[:1], TD.E2E["G"], "masks", sigma_rel=TD.E2E["sigma"])
    loss, out, winner = R.pointcloud_project_loss(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2], gt=gm,
                                                  num_candidates=2)
    assert winner.cpu().tolist() == ref["winner"].tolist()
    close(loss, ref["losses"]["proj"], what="min-of-2 loss on prepared masks")
    loss.backward()
    check_grads(leaves[:3], ref["grads"]["proj"][:3], "min-of-2", ("points", "quaternions", "s"))
    # full-size masks with the key are refused, on the device too
    with pytest.raises(NotImplementedError, match="smooth_gt"):
        R.pointcloud_project_loss(cfg, leaves[0], leaves[1], None, None, kern, scaling_factor=leaves[2], gt=masks[:1], num_candidates=2)


# ------------------------------------------------------------------------------------------------ 3. the training step
class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def f10():
    cfg = Cfg(json.load(open(os.path.join(GOLDEN, "f10_config.json"))))
    g = np.load(os.path.join(GOLDEN, "f10_full_step.npz"))
    state = {k[len("state/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}
    return cfg, torch.from_numpy(g["images"]).cuda(), torch.from_numpy(g["masks"]).cuda(), state


def test_eager_step_with_the_key_is_the_composition(f10):
    """The step with cfg.pc_gauss_filter_gt equals the step without it fed the prepared masks (the same kernels: equal bits),
    agrees with the step fed the ORACLE's smoothed masks under the parity rule, and differs from the step on the raw masks."""
    import dpc.render as R
    from dpc.harness import TrainStep

    cfg, images, masks, state = f10
    on = Cfg(cfg, pc_gauss_filter_gt=True)
    dev = torch.device("cuda")
    plain, keyed = TrainStep(cfg, dev), TrainStep(on, dev)
    plain.load_reference_state(state)
    keyed.load_reference_state(state)
    sigma = R.get_smooth_sigma(cfg, 7)
    total, out = keyed.loss(images, masks, global_step=7)
    prepared = R.smooth_gt(on, masks, cfg.vox_size, "masks", sigma_rel=sigma)
    assert torch.equal(out["pooled_masks"], prepared)
    assert torch.equal(total, plain.loss(images, prepared, global_step=7)[0])
    oracle = GO.smooth_gt(masks.cpu().numpy(), 1, True, masks.shape[2] // cfg.vox_size, "mean", taps32(cfg.pc_gauss_kernel_size, sigma))
    ref = plain.loss(images, torch.from_numpy(oracle).float().cuda(), global_step=7)[0]
    close(total, ref, what="step loss: the node vs the oracle's masks")
    raw = float(plain.loss(images, masks, global_step=7)[0].detach())
    assert abs(float(total.detach()) - raw) > 1e-3 * abs(raw), (float(total.detach()), raw)


def test_captured_step_follows_sigma_and_the_switch_off(f10):
    """A captured step with the key and the switch-off, replayed while sigma_rel falls through 1.0: every replay's loss equals
    the eager step's of the same global_step (the tolerance of tests/test_harness.py::test_captured_step_matches_eager), and
    the graph is captured again only where the projection's tap window changes -- never for the threshold."""
    import dpc.render as R
    from dpc.harness import TrainStep

    cfg, images, masks, state = f10
    cfg = Cfg(cfg, pc_gauss_filter_gt=True, pc_gauss_filter_gt_switch_off=True, pc_point_dropout=1.0, max_number_of_steps=25)
    dev = torch.device("cuda")

    def make(capturable):
        step = TrainStep(cfg, dev, lr=1e-4, device_dropout=True, capturable=capturable)
        step.load_reference_state(state)
        return step

    eager, captured = make(False), make(True)
    replay = captured.capture(images, masks, warmup=2)
    for _ in range(2):
        eager(images, masks)
    le, lc, sigmas, buckets, recaptures = [], [], [], [], []
    for _ in range(11):
        sigma = R.get_smooth_sigma(cfg, eager.global_step)
        sigmas.append(sigma)
        buckets.append(R.taps_bucket(R.smoothing_kernel(cfg, sigma)[0]))
        le.append(float(eager(images, masks)))
        lc.append(float(replay(images, masks)))
        recaptures.append(captured.recaptures)
    assert sigmas[0] > 1.3 and sigmas[-1] < 0.95 and all(abs(s - 1.0) > 1e-3 for s in sigmas)
    cross = next(i for i, s in enumerate(sigmas) if s < 1.0)
    assert 0 < cross < len(sigmas) - 1
    assert np.allclose(le, lc, rtol=1e-4), (le, lc)
    for (name, p), q in zip(eager.nets.named_parameters(), captured.nets.parameters()):
        assert float((p.detach() - q.detach()).abs().max()) < 1e-4, name
    changes = [i for i in range(1, len(buckets)) if buckets[i] != buckets[i - 1]]
    assert captured.recaptures == len(changes), (captured.recaptures, buckets)
    if cross not in changes:
        assert recaptures[cross] == recaptures[cross - 1]
    # the switch acts: at the first step below 1 the eager loss is the loss on the pooled masks, not on smoothed ones
    step = eager.global_step - (len(sigmas) - cross)
    probe = make(False)
    off = float(probe.loss(images, masks, global_step=step)[0].detach())
    probe.cfg = Cfg(cfg, pc_gauss_filter_gt_switch_off=False)
    assert abs(off - float(probe.loss(images, masks, global_step=step)[0].detach())) > 1e-4 * abs(off)
