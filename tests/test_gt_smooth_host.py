"""The smoothed ground truth (cfg.pc_gauss_filter_gt, pc_gauss_filter_gt_rgb, pc_gauss_filter_gt_switch_off) without a GPU: the
fp64 oracle of tests/gt_smooth_oracle.py against F27 (the reference's taps, numpy restatements of its TF-1 lines,
tests/golden/make_golden_gt_smooth.py) and against torch's conv2d, the C ABI's argument checks, the refusals of the losses,
the CPU route of dpc.render.smooth_gt, and the training step's wiring."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gt_smooth_oracle as GO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpc_render.h")

# name -> (channels, planar, factor, resize mode)
F27_CASES = {"masks": (1, True, 2, "mean"), "images": (3, False, 1, "sample"), "depths": (1, False, 2, "sample")}


def f27():
    return dict(np.load(os.path.join(GOLDEN, "f27_gt_smooth.npz")))


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("name", sorted(F27_CASES))
def test_oracle_reproduces_the_reference(name):
    g = f27()
    C, planar, f, mode = F27_CASES[name]
    lo, hi = (g["depths_remap"] if name == "depths" else (0.0, 0.0))
    got = GO.smooth_gt(g[name + "_in"], C, planar, f, mode, g[name + "_taps"], lo, hi)
    assert got.shape == g[name + "_out"].shape and float(np.abs(got - g[name + "_out"]).max()) <= 1e-12
    assert float(np.abs(GO.resized_only(g[name + "_in"], C, planar, f, mode, lo, hi) - g[name + "_resized"]).max()) == 0.0
    # the fixture reaches what it is meant to
    assert g["masks_taps"].size == 11 and g["masks_out"].shape == (2, 8, 8, 1) and g["images_out"].shape == (2, 6, 10, 3)
    assert g["depths_in"][0, 4, 4, 0] == 10.0 and g["depths_in"][0, 4, 6, 0] == 2.25 and g["depths_resized"].max() == 5.0
    # SAME pads with zeros: a constant plane darkens at the border
    flat = GO.smooth_gt(np.ones((1, 1, 8, 8)), 1, True, 1, "sample", g["masks_taps"])
    assert flat[0, 0, 0, 0] < 0.5 and flat[0, 4, 4, 0] > flat[0, 0, 4, 0]


@pytest.mark.parametrize("C,planar,f,mode,n,remap", [(1, True, 2, "mean", 11, None), (3, False, 1, "sample", 5, None),
                                                     (3, True, 3, "sample", 7, None), (1, False, 2, "sample", 7, (10.0, 5.0)),
                                                     (1, True, 1, "mean", 63, None)])
def test_oracle_against_conv2d(C, planar, f, mode, n, remap):
    """The same definition stated independently: avg_pool2d or strided sampling, then conv2d in fp64 with groups=C and zero
    padding fsz // 2 -- within 1e-12."""
    rng = np.random.RandomState(n + C)
    H, W = 9, 14
    gt = rng.rand(2, C, f * H, f * W) if planar else rng.rand(2, f * H, f * W, C)
    if remap:
        gt[rng.rand(*gt.shape) < 0.3] = remap[0]
    taps = GO.gauss_kernel_1d(n, 1.3)
    t = torch.from_numpy(gt if planar else np.moveaxis(gt, 3, 1).copy())
    if remap:
        t = torch.where(t == remap[0], torch.full_like(t, remap[1]), t)
    t = F.avg_pool2d(t, f) if (mode == "mean" and f > 1) else t[:, :, ::f, ::f]
    w = torch.from_numpy(taps)
    t = F.conv2d(t.contiguous(), w.reshape(1, 1, 1, n).repeat(C, 1, 1, 1), padding=(0, n // 2), groups=C)
    t = F.conv2d(t, w.reshape(1, 1, n, 1).repeat(C, 1, 1, 1), padding=(n // 2, 0), groups=C)
    ref = t.permute(0, 2, 3, 1).numpy()
    got = GO.smooth_gt(gt, C, planar, f, mode, taps, *(remap or (0.0, 0.0)))
    assert float(np.abs(got - ref).max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ 2. the C ABI
def _call(L, gt=1, S=2, C=1, Hs=16, Ws=16, planar=1, H=8, W=8, mode=0, lo=0.0, hi=0.0, host=1, dev=None, n=11, out=1):
    """dpc_gt_smooth with dummy non-NULL addresses: every check below fails before anything is launched or read."""
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    return L.dpc_gt_smooth(addr if gt else None, S, C, Hs, Ws, planar, H, W, mode, lo, hi, addr if host else None,
                           addr if dev else None, n, addr if out else None, None)


def test_argument_checks_need_no_device():
    from dpc.render import _native

    L = _native.lib()
    N = _native
    assert _call(L, gt=0) == N.DPC_ERR_NULL and _call(L, out=0) == N.DPC_ERR_NULL
    assert _call(L, host=0, dev=None) == N.DPC_ERR_NULL          # neither tap source
    for bad in (dict(S=0), dict(S=-1), dict(C=2), dict(C=0), dict(C=4), dict(Hs=12), dict(Hs=16, Ws=24, W=8), dict(Hs=4, Ws=4),
                dict(H=0), dict(mode=2), dict(mode=-1), dict(Hs=2048, Ws=2048, H=1024, W=1024), dict(Hs=1025, Ws=1025, H=1025, W=1025)):
        assert _call(L, **bad) == N.DPC_ERR_SHAPE, bad
    for n in (0, -1, 2, 10, 64, 65):
        assert _call(L, n=n) == N.DPC_ERR_TAPS, n
    assert N.DPC_MAX_TAPS == 63 and (N.DPC_GT_RESIZE_MEAN, N.DPC_GT_RESIZE_SAMPLE) == (0, 1)


def test_header_binding_and_abi():
    from dpc.render import _native

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+dpc_gt_smooth\s*\(", text)
    assert "dpc_gt_smooth" in _native.SYMBOLS
    proto = re.search(r"dpc_gt_smooth\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    (_, _, argtypes), = [f for f in _native._FUNCTIONS if f[0] == "dpc_gt_smooth"]
    assert len(argtypes) == len(proto.split(",")) == 16
    assert "#define DPC_GT_RESIZE_MEAN 0" in text and "#define DPC_GT_RESIZE_SAMPLE 1" in text
    assert _native.ABI_VERSION == 15 and _native.lib().dpc_abi_version() == 15 and "#define DPC_ABI_VERSION 15" in text
    makefile = open(os.path.join(os.path.dirname(_native.LIB_PATH), "Makefile")).read()
    assert "dpc_gt_smooth.hip" in makefile


# ------------------------------------------------------------------------------------------------ 3. dpc.render
def _outputs(S=2, G=8, **lazy):
    import dpc.render as R

    entries = {"tr_pc": torch.zeros(S, 5, 3), "voxels": torch.zeros(S, G, G, G, 1)}
    entries.update(lazy)
    return R.ProjectionOutputs(torch.zeros(S, G, G, 1), lambda: entries)


def test_the_four_refusals_still_raise_without_gt_prepared():
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    out, rgb = _outputs(), torch.zeros(2, 5, 3)
    on, on_rgb = chair_unsupervised(vox_size=8, pc_gauss_filter_gt=True), chair_unsupervised(vox_size=8, pc_gauss_filter_gt_rgb=True)
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt.*smooth_gt"):
        R.proj_depth_loss(on, out, torch.zeros(2, 8, 8, 1))
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt.*smooth_gt"):
        R.drc_loss(on, out, torch.zeros(2, 1, 8, 8))
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt_rgb.*smooth_gt"):
        R.proj_rgb_loss(on_rgb, out, rgb, torch.zeros(2, 8, 8, 3))
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt_rgb"):
        R.drc_rgb_loss(on_rgb, out, rgb, torch.zeros(2, 8, 8, 3))
    # prepared ground truth must be what smooth_gt returns for this projection
    with pytest.raises(ValueError, match="gt_prepared"):
        R.drc_loss(on, out, torch.zeros(2, 1, 8, 8), gt_prepared=True)
    with pytest.raises(ValueError, match="gt_prepared"):
        R.proj_depth_loss(on, out, torch.zeros(2, 16, 16, 1), gt_prepared=True)
    with pytest.raises(ValueError, match="gt_prepared"):
        R.proj_rgb_loss(on_rgb, out, rgb, torch.zeros(2, 3, 8, 8), gt_prepared=True)
    assert {"smooth_gt", "gauss_smoothen_image", "DeviceTaps"} <= set(R.__all__)


def test_prepared_ground_truth_reaches_the_staged_losses_unchanged():
    """gt_prepared on outputs of the staged fallback (torch route, no device): read as it is, no remap of max_dataset_depth."""
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    g = torch.Generator().manual_seed(2)
    cfg = chair_unsupervised(vox_size=4, pc_gauss_filter_gt=True, max_depth=5.0, max_dataset_depth=10.0)
    depth = torch.rand(2, 4, 4, 1, generator=g, dtype=torch.float64)
    gt = torch.rand(2, 4, 4, 1, generator=g, dtype=torch.float64)
    gt[0, 0, 0, 0] = 10.0   # stays 10: the remap ran before the smoothing, inside smooth_gt
    got = R.proj_depth_loss(cfg, _outputs(G=4, proj_depth=depth), gt, gt_prepared=True)
    assert abs(got.item() - 0.5 * ((gt - depth) ** 2).sum().item() / 2) <= 1e-12
    probs = torch.rand(5, 2, 4, 4, 1, generator=g, dtype=torch.float64)
    got = R.drc_loss(cfg, _outputs(G=4, drc_probs=probs), gt, gt_prepared=True)
    p = probs[..., 0]
    ref = ((1.0 - gt[..., 0]) * p[:-1].sum(0) + gt[..., 0] * p[-1]).sum() / 2
    assert abs(got.item() - ref.item()) <= 1e-12 * abs(ref.item())


def test_full_size_masks_with_the_key_are_refused():
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    on = chair_unsupervised(vox_size=8, pc_gauss_filter_gt=True)
    pred, full = torch.zeros(2, 8, 8, 1), torch.zeros(2, 1, 16, 16)
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt.*smooth_gt"):
        R.silhouette_loss(pred, full, 1, None, cfg=on)
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt.*smooth_gt"):
        R.pointcloud_project_loss(on, torch.zeros(2, 4, 3), torch.zeros(2, 4), None, None, None, gt=full)
    # masks at the silhouette's size pass the check (the device check speaks next: these are CPU tensors)
    with pytest.raises(RuntimeError, match="MI355X"):
        R.silhouette_loss(pred, torch.zeros(2, 8, 8, 1), 1, None, cfg=on)
    with pytest.raises(RuntimeError, match="MI355X"):
        R.silhouette_loss(pred, full, 1, None, cfg=chair_unsupervised(vox_size=8))


@pytest.mark.parametrize("name", sorted(F27_CASES))
def test_cpu_route_of_smooth_gt(name):
    """CPU tensors: the same rule with torch ops, against F27 under the parity rule; every accepted layout gives equal bits."""
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    g = f27()
    sigma = {"masks": 1.0, "images": 0.8, "depths": 1.5}[name]
    cfg = chair_unsupervised(vox_size=8, pc_gauss_kernel_size=int(g[name + "_taps"].size), max_depth=5.0, max_dataset_depth=10.0)
    gt, ref = torch.from_numpy(g[name + "_in"]), g[name + "_out"]
    size = ref.shape[1:3]
    got = R.smooth_gt(cfg, gt, size, name, sigma_rel=sigma)
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape and not got.requires_grad
    assert float(np.abs(got.double().numpy() - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    layouts = {"masks": [gt[:, 0], gt.permute(0, 2, 3, 1)], "images": [gt.permute(0, 3, 1, 2).contiguous()],
               "depths": [gt[..., 0], gt.permute(0, 3, 1, 2)]}[name]
    for other in layouts:
        assert torch.equal(R.smooth_gt(cfg, other, size, name, sigma_rel=sigma), got), tuple(other.shape)
    # taps from a smoothing_kernel list: the same kernel, the same bits
    assert torch.equal(R.smooth_gt(cfg, gt, size, name, kernel=R.smoothing_kernel(cfg, sigma)), got)


def test_smooth_gt_switch_off_sources_and_errors():
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.step import pooled_masks

    g = f27()
    masks, depths = torch.from_numpy(g["masks_in"]), torch.from_numpy(g["depths_in"])
    off = chair_unsupervised(vox_size=8, pc_gauss_kernel_size=11, pc_gauss_filter_gt_switch_off=True, max_depth=5.0, max_dataset_depth=10.0)
    assert torch.equal(R.smooth_gt(off, masks, 8, "masks", sigma_rel=0.99), pooled_masks(masks, 8))   # the resized bits
    at_one = R.smooth_gt(off, masks, 8, "masks", sigma_rel=1.0)
    assert float(np.abs(at_one.double().numpy() - g["masks_out"]).max()) <= 1e-5            # tf.less: 1.0 is smoothed
    assert not torch.equal(at_one, pooled_masks(masks, 8))
    # depth has no switch-off (losses.py:128-129)
    d = R.smooth_gt(off, depths, 6, "depths", sigma_rel=0.5)
    ref = GO.smooth_gt(g["depths_in"], 1, False, 2, "sample", R.gauss_kernel_1d(11, 0.5).numpy(), 10.0, 5.0)
    assert float(np.abs(d.double().numpy() - ref).max()) <= 1e-5 * 5.0 and float(np.abs(ref - g["depths_resized"]).max()) > 1e-2
    cfg = chair_unsupervised(vox_size=8, pc_gauss_kernel_size=11)
    for bad in (dict(), dict(sigma_rel=1.0, kernel=R.smoothing_kernel(cfg, 1.0))):
        with pytest.raises(ValueError, match="exactly one"):
            R.smooth_gt(cfg, masks, 8, "masks", **bad)
    with pytest.raises(ValueError, match="kind"):
        R.smooth_gt(cfg, masks, 8, "mask", sigma_rel=1.0)
    with pytest.raises(ValueError, match="integer multiple"):
        R.smooth_gt(cfg, masks, 6, "masks", sigma_rel=1.0)
    with pytest.raises(ValueError, match="images must be"):
        R.smooth_gt(cfg, masks, 8, "images", sigma_rel=1.0)
    with pytest.raises(ValueError, match="1024"):
        R.smooth_gt(cfg, torch.zeros(1, 1, 2048, 2048), 1024, "masks", sigma_rel=1.0)
    img = torch.rand(2, 8, 8, 3, generator=torch.Generator().manual_seed(0))
    ref = GO.smooth_gt(img.numpy(), 3, False, 1, "sample", R.gauss_kernel_1d(11, 1.2).numpy())
    assert float(np.abs(R.gauss_smoothen_image(cfg, img, 1.2).double().numpy() - ref).max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. the training step
def _step(**kw):
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.step import TrainStep

    cfg = chair_unsupervised(batch_size=1, step_size=2, vox_size=32, pc_num_points=64, pose_predictor_student=False,
                             pc_point_dropout=1.0, pc_relative_sigma=2.0, pc_relative_sigma_end=0.5, max_number_of_steps=100,
                             input_shape=[64, 64, 3], saved_depth=True, **kw)
    torch.manual_seed(0)
    return cfg, TrainStep(cfg, torch.device("cpu"))


def test_train_step_prepares_the_ground_truth_once_per_kind(monkeypatch):
    """With the keys set: one smooth_gt call per ground-truth kind with THIS step's sigma_rel, the same tensor reaches the
    silhouette loss, drc_loss and out["pooled_masks"], the prepared depths and images reach their losses with gt_prepared.
    The renderer is replaced by stand-ins: this runs without a device."""
    import dpc.harness.step as S
    import dpc.render as R

    calls, seen = [], {}
    real_smooth = R.smooth_gt

    def smooth(cfg, gt, size, kind, sigma_rel=None, kernel=None, schedule=None):
        calls.append((kind, sigma_rel, size, kernel, schedule))
        return real_smooth(cfg, gt, size, kind, sigma_rel=sigma_rel, kernel=kernel, schedule=schedule)   # the CPU route

    def project(cfg, pc, q, t, rgb, kernel, **kw):
        proj = pc.sum().reshape(1, 1, 1, 1).expand(q.shape[0], 32, 32, 1) * 0.0
        return R.ProjectionOutputs(proj, lambda: {})

    def silhouette(pred, gt, K, w=None):
        seen["silhouette"] = gt
        return pred.sum() + 1.0, torch.zeros(gt.shape[0], dtype=torch.int32)

    def drc(cfg, outputs, masks, w=None, gt_prepared=False):
        seen["drc"] = (masks, gt_prepared)
        return outputs["proj"].sum() + 3.0

    def depth(cfg, outputs, depths, w=None, return_depth=False, gt_prepared=False):
        seen["depth"] = (depths, gt_prepared)
        return outputs["proj"].sum() + 5.0, None

    def proj_rgb(cfg, outputs, all_rgb, images, kernel=None, w=None, return_rgb=False, grids=None, gt_prepared=False):
        seen["rgb"] = (images, gt_prepared)
        return all_rgb.sum() * 0.0 + 7.0, None

    def fused(cfg, pc, q, t, rgb, kernel=None, scaling_factor=None, gt=None, num_candidates=1, **kw):
        seen["fused"] = (gt, num_candidates)
        proj = pc.sum().reshape(1, 1, 1, 1).expand(q.shape[0], 32, 32, 1) * 0.0
        return proj.sum() + 2.0, {"proj": proj}, torch.zeros(gt.shape[0], dtype=torch.int32)

    for name, fn in (("smooth_gt", smooth), ("pointcloud_project_fast", project), ("silhouette_loss", silhouette), ("drc_loss", drc),
                     ("proj_depth_loss", depth), ("proj_rgb_loss", proj_rgb), ("rgb_grids", lambda *a, **k: "shared"),
                     ("pointcloud_project_loss", fused)):
        monkeypatch.setattr(S.R, name, fn)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 64, 64, generator=g)
    masks = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float()
    depths = 1.5 + torch.rand(2, 64, 64, 1, generator=g)

    # nodes on one projection: masks, depths and images, each prepared once with the sigma of step 40
    cfg, step = _step(pose_predict_num_candidates=1, drc_weight=0.5, proj_depth_weight=0.25, pc_rgb=True, proj_rgb_weight=2.0,
                      pc_gauss_filter_gt=True, pc_gauss_filter_gt_rgb=True)
    total, out = step.loss(images, masks, global_step=40, depths=depths)
    sigma = R.get_smooth_sigma(cfg, 40)
    assert abs(sigma - 1.4) < 1e-12
    assert sorted(c[0] for c in calls) == ["depths", "images", "masks"]
    assert all(c[1] == sigma and c[2] == 32 and c[3] is None and c[4] is None for c in calls)
    prepared = seen["silhouette"]
    assert tuple(prepared.shape) == (2, 32, 32, 1) and seen["drc"][0] is prepared and out["pooled_masks"] is prepared
    assert seen["drc"][1] is True and seen["depth"][1] is True and seen["rgb"][1] is True
    assert tuple(seen["depth"][0].shape) == (2, 32, 32, 1) and tuple(seen["rgb"][0].shape) == (2, 32, 32, 3)
    assert torch.equal(prepared, real_smooth(cfg, masks, 32, "masks", sigma_rel=sigma))
    assert not torch.equal(prepared, S.pooled_masks(masks, 32))
    assert abs(total.item() - (1.0 + 0.25 * 5.0 + 0.5 * 3.0 + 2.0 * 7.0)) < 1e-12
    for capture in (step.capture, step.capture_compute):
        with pytest.raises(NotImplementedError, match="eager only"):
            capture(images, masks)

    # global_step of the step itself when none is given
    calls.clear()
    step.global_step = 80
    step.loss(images, masks, depths=depths)
    assert {c[1] for c in calls} == {R.get_smooth_sigma(cfg, 80)}

    # the one-node path, K candidates: the prepared masks are the fused loss's ground truth
    calls.clear()
    cfg, step = _step(pose_predict_num_candidates=4, pc_gauss_filter_gt=True, pc_gauss_filter_gt_switch_off=True)
    total, out = step.loss(images, masks, global_step=90)   # sigma 0.65 < 1: switched off, the pooled bits
    assert [c[0] for c in calls] == ["masks"] and calls[0][1] == R.get_smooth_sigma(cfg, 90) < 1.0
    assert seen["fused"][1] == 4 and seen["fused"][0] is out["pooled_masks"]
    assert torch.equal(seen["fused"][0], S.pooled_masks(masks, 32))
    step.loss(images, masks, global_step=10)                # sigma 1.85: smoothed
    assert not torch.equal(seen["fused"][0], S.pooled_masks(masks, 32))

    # only the rgb key: masks stay as they are, images are prepared
    calls.clear()
    cfg, step = _step(pose_predict_num_candidates=1, pc_rgb=True, proj_rgb_weight=2.0, pc_gauss_filter_gt_rgb=True)
    total, out = step.loss(images, masks, global_step=0)
    assert [c[0] for c in calls] == ["images"] and seen["silhouette"] is masks
    assert torch.equal(out["pooled_masks"], S.pooled_masks(masks, 32))

    # without the keys nothing is prepared
    calls.clear()
    cfg, step = _step(pose_predict_num_candidates=1)
    step.loss(images, masks)
    assert calls == [] and seen["fused"][0] is masks


def test_train_step_refuses_the_rgb_key_with_the_drc_colour_loss():
    cfg, step = _step(pose_predict_num_candidates=1, pc_rgb=True, drc_rgb_weight=0.5, pc_gauss_filter_gt_rgb=True)
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt_rgb.*drc_rgb_weight"):
        step.loss(torch.zeros(2, 3, 64, 64), torch.zeros(2, 1, 64, 64))


def test_exact_path_takes_prepared_masks(monkeypatch):
    import dpc.harness.step as S
    import dpc.render as R

    seen = {}

    def exact(cfg, pc, q, sigma):
        return pc.sum().reshape(1, 1, 1, 1).expand(q.shape[0], 32, 32, 1) * 0.0, None

    def silhouette(pred, gt, K, w=None):
        seen["gt"] = gt
        return pred.sum() + 1.0, torch.zeros(gt.shape[0], dtype=torch.int32)

    monkeypatch.setattr(S.R, "pointcloud_project_exact", exact)
    monkeypatch.setattr(S.R, "silhouette_loss", silhouette)
    cfg, step = _step(pose_predict_num_candidates=1, pc_fast=False, pc_gauss_filter_gt=True)
    masks = (torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(1)) > 0.5).float()
    _, out = step.loss(torch.zeros(2, 3, 64, 64), masks, global_step=20)
    assert out["pooled_masks"] is seen["gt"]
    assert torch.equal(seen["gt"], R.smooth_gt(cfg, masks, 32, "masks", sigma_rel=R.get_smooth_sigma(cfg, 20)))


def test_captured_gt_taps_follow_sigma_and_the_switch():
    """The taps a captured step writes in front of a replay: this step's Gaussian, the identity kernel while switched off."""
    import dpc.render as R

    cfg, step = _step(pose_predict_num_candidates=1, pc_gauss_filter_gt=True, pc_gauss_filter_gt_switch_off=True)
    n = int(cfg.pc_gauss_kernel_size)
    assert np.array_equal(step._gt_tap_values(10), R.gauss_kernel_1d(n, R.get_smooth_sigma(cfg, 10)).numpy())
    ident = step._gt_tap_values(90)
    assert ident.size == n and ident[n // 2] == 1.0 and np.count_nonzero(ident) == 1
    cfg, step = _step(pose_predict_num_candidates=1, pc_gauss_filter_gt=True)
    assert np.array_equal(step._gt_tap_values(90), R.gauss_kernel_1d(n, R.get_smooth_sigma(cfg, 90)).numpy())
    cfg, step = _step(pose_predict_num_candidates=1)
    assert step._new_gt_taps(0) is None
