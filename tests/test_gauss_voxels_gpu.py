"""The exact Gaussian occupancy renderer (cfg.pc_fast == false) on the device, against the fp64 oracle of
tests/gauss_voxels_oracle.py (the literal broadcast form of dpc/util/point_cloud.py:17-57, 219-226).

Parity rule of the project: max|dev - ref| <= 1e-5 * max(1, max|ref|), for raw, the clipped grid and the gradient.

The cases are the smallest that can still break the kernels: G = 17 and 24 (32 x 32 tiles partly dead, an odd width that the
backward pads to its compiled width), G = 32 and 64 (the production widths, one and four planes per wave), G = 40 (the
four-plane forward and the 64-wide backward with dead rows and columns), N = 1, 257 and 0 around the forward's 128-point chunk and
the backward's 128-point workgroup, B = 3, the three normalisation modes, sigma_rel 3, 1 and 0.5, and clouds with points on
the cube's faces, between the cube and the grid's edge, and beyond +-1.

The clip mask.  Every case asserts on the oracle that no raw value lies within 1e-6 of 1 and that none is negative.  Towards
0 nothing more can be asked: raw is a sum of positive terms, so in fp64 it is tiny but not zero wherever the exponent stays
above exp's underflow at about -745 (the fixture's smallest value is 8.7e-46), exactly 0 only beyond that, and "no value
within 1e-6 of 0" cannot hold for any cloud.  It need not: the pass-through set 0 <= raw <= 1 is inclusive and the kernels'
raw is a sum of non-negative fp32 products, so a value near 0 is inside the set on both sides whatever the rounding; only
the upper edge can be crossed.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gauss_voxels_oracle as GO

pytestmark = pytest.mark.gpu

TOL = 1e-5
#        tag            B  N    G   sigma_rel mode          seed
CASES = [("g17", 1, 64, 17, 1.0, GO.ANALYTICAL, 1),
         ("g24_n257", 1, 257, 24, 1.0, GO.PER_POINT, 2),
         ("g32_b3", 3, 64, 32, 3.0, GO.ANALYTICAL, 3),
         ("g64", 1, 64, 64, 3.0, GO.NONE, 4),
         ("g64_narrow", 1, 64, 64, 0.5, GO.ANALYTICAL, 5),
         ("g40", 1, 64, 40, 1.0, GO.PER_POINT, 6),
         ("g17_n1", 1, 1, 17, 0.5, GO.NONE, 7),
         ("g24_n129_b3", 3, 129, 24, 0.5, GO.NONE, 8),
         ("g32_wide_none", 1, 64, 32, 3.0, GO.NONE, 9)]
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_data(tag):
    """Inputs and the oracle's answers of a case, computed once and shared (read only)."""
    _, B, N, G, sigma_rel, mode, seed = next(c for c in CASES if c[0] == tag)
    rng = np.random.default_rng(seed)
    tr = GO.points(rng, B, N)
    dvox = rng.standard_normal((B, G, G, G)).astype(np.float32)
    sigma = sigma_rel / G
    raw = GO.raw_separable(tr, G, sigma, mode)
    lo, near1 = GO.clip_margin(raw)
    assert lo >= 0.0 and near1 > 1e-6, "case %s: the clip mask cannot be told in fp32 (min raw %g, min |raw - 1| %g)" % (tag, lo, near1)
    return dict(B=B, N=N, G=G, sigma=sigma, mode=mode, tr=tr, dvox=dvox, raw=raw, vox=np.clip(raw, 0.0, 1.0),
                dtr=GO.grad_separable(tr, G, sigma, mode, dvox, raw))


def close(dev, ref, what):
    dev = dev.detach().double().cpu().numpy() if isinstance(dev, torch.Tensor) else np.asarray(dev, dtype=np.float64)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    err = float(np.abs(dev - ref).max()) if ref.size else 0.0
    print("%s: max|dev - ref| = %.3e, bound %.3e (%.2f of it)" % (what, err, TOL * scale, err / (TOL * scale)))
    assert err <= TOL * scale, "%s: max|dev - ref| = %.3e > %.3e" % (what, err, TOL * scale)


def c_abi(c, tr, dvox):
    """(raw, vox, dtr) straight from the two entry points."""
    from dpc.render import _native as N

    P = N.DpcParams(c["B"], c["N"], c["G"], c["G"], c["G"], 0, 0, 2.0, 1.875, 1e-5, 10.0, 1)
    shape = (c["B"], c["G"], c["G"], c["G"])
    raw, vox = torch.full(shape, np.nan, device="cuda"), torch.full(shape, np.nan, device="cuda")
    dtr = torch.full((c["B"], c["N"], 3), np.nan, device="cuda")
    st = N.stream_ptr(tr.device)
    N.check(N.lib().dpc_gauss_voxels_fwd(ctypes.byref(P), N.ptr(tr), c["sigma"], c["mode"], N.ptr(raw), N.ptr(vox), st), "fwd")
    N.check(N.lib().dpc_gauss_voxels_bwd(ctypes.byref(P), N.ptr(tr), c["sigma"], c["mode"], N.ptr(raw), N.ptr(dvox), N.ptr(dtr), st),
            "bwd")
    torch.cuda.synchronize()
    return raw, vox, dtr


def mode_cfg(G, mode, **kw):
    from oracle import dpc_oracle as O

    return O.Cfg(vox_size=G, pc_normalise_gauss=mode == GO.PER_POINT, pc_normalise_gauss_analytical=mode == GO.ANALYTICAL, **kw)


@pytest.mark.parametrize("tag", IDS)
def test_entry_points_match_the_oracle_and_repeat_bit_for_bit(tag):
    c = case_data(tag)
    tr, dvox = torch.from_numpy(c["tr"]).cuda(), torch.from_numpy(c["dvox"]).cuda()
    raw, vox, dtr = c_abi(c, tr, dvox)
    close(raw, c["raw"], tag + " raw")
    close(vox, c["vox"], tag + " vox")
    close(dtr, c["dtr"], tag + " dtr")
    mask_dev = ((raw >= 0) & (raw <= 1)).cpu().numpy()
    assert np.array_equal(mask_dev, (c["raw"] >= 0) & (c["raw"] <= 1)), "the pass-through set differs from the oracle's"
    raw2, vox2, dtr2 = c_abi(c, tr, dvox)
    assert torch.equal(raw, raw2) and torch.equal(vox, vox2), "two runs of the forward differ"
    assert torch.equal(dtr, dtr2), "two runs of the backward differ"


@pytest.mark.parametrize("tag", ["g17", "g24_n257", "g64_narrow"])
def test_pointcloud2voxels_layout_and_autograd(tag):
    import dpc.render as R

    c = case_data(tag)
    cfg = mode_cfg(c["G"], c["mode"])
    tr = torch.from_numpy(c["tr"]).cuda().requires_grad_(True)
    out = R.pointcloud2voxels(cfg, tr, c["sigma"])
    assert out.shape == (c["B"], c["G"], c["G"], c["G"], 1)
    assert out._base is not None and not out.is_contiguous(), "the reference's layout is a transposed view, not a copy"
    _, literal = GO.pointcloud2voxels_literal(c["tr"], c["G"], c["sigma"], c["mode"])   # the literal form decides the axes
    close(out, literal, tag + " voxels in the reference's layout")
    dvox = torch.from_numpy(c["dvox"]).cuda()
    (out[..., 0].transpose(1, 2) * dvox).sum().backward()
    close(tr.grad, c["dtr"], tag + " d(points) through autograd")
    with torch.no_grad():
        again = R.pointcloud2voxels(cfg, tr, c["sigma"])
    assert torch.equal(again, out)


def test_no_points_gives_a_zero_grid_and_an_empty_gradient():
    import dpc.render as R

    cfg = mode_cfg(17, GO.ANALYTICAL)
    tr = torch.zeros((2, 0, 3), device="cuda", requires_grad=True)
    out = R.pointcloud2voxels(cfg, tr, 1.0 / 17)
    assert out.shape == (2, 17, 17, 17, 1) and float(out.detach().abs().max()) == 0.0
    out.sum().backward()
    assert tr.grad.shape == (2, 0, 3)
    none = R.pointcloud2voxels(cfg, torch.zeros((0, 5, 3), device="cuda"), 1.0 / 17)
    assert none.shape == (0, 17, 17, 17, 1)


def test_launches_are_named_in_the_profile_record():
    import dpc.render as R
    from dpc.render import _native as N

    c = case_data("g17")
    big = case_data("g40")

    def run():
        for d in (c, big):
            tr = torch.from_numpy(d["tr"]).cuda().requires_grad_(True)
            R.pointcloud2voxels(mode_cfg(d["G"], d["mode"]), tr, d["sigma"]).sum().backward()

    assert N.launched_instantiations(run, torch.device("cuda", 0)) == {
        "k_gauss_voxels_fwd<1>", "k_gauss_voxels_bwd<16>", "k_gauss_voxels_fwd<4>", "k_gauss_voxels_bwd<32>"}


def test_pointcloud_project_exact_against_the_fixture(golden):
    import dpc.render as R

    g = golden("f23_gauss_voxels.npz")
    cfg = mode_cfg(int(g["voxels"].shape[1]), GO.ANALYTICAL)
    pc = torch.from_numpy(g["pc"]).cuda().requires_grad_(True)
    q = torch.from_numpy(g["q"]).cuda().requires_grad_(True)
    proj, voxels = R.pointcloud_project_exact(cfg, pc, q, float(g["sigma"]))
    close(proj, g["proj"], "proj")
    close(voxels, g["voxels"], "voxels")
    ((voxels * torch.from_numpy(g["dvox"]).cuda().float()).sum() + (proj * torch.from_numpy(g["dproj"]).cuda().float()).sum()).backward()
    close(pc.grad, g["dpc"], "d(points)")
    close(q.grad, g["dq"], "d(quaternion)")


def _step_cfg(**kw):
    from dpc.harness import chair_unsupervised

    base = dict(vox_size=16, pc_num_points=96, pc_fast=False, pose_predict_num_candidates=2, batch_size=1, step_size=2,
                pc_point_dropout=1.0, input_shape=[32, 32, 3])
    base.update(kw)
    return chair_unsupervised(**base)


def test_train_step_without_pc_fast_is_the_composition_done_by_hand():
    import dpc.render as R
    from dpc.harness import TrainStep
    from dpc.harness.step import student_loss

    cfg = _step_cfg()
    torch.manual_seed(5)
    step = TrainStep(cfg, "cuda")
    g = torch.Generator().manual_seed(6)
    images = torch.rand(2, 3, 32, 32, generator=g).cuda()
    masks = (torch.rand(2, 1, 32, 32, generator=g) > 0.5).float().cuda()
    total, out = step.loss(images, masks, global_step=1000)
    # by hand: model_pc.py:233-252 and get_loss with the pieces of the public interface
    pred = step.predict(images)
    K, V = 2, 2
    points = pred["points_1"].repeat_interleave(V * K, dim=0)
    sigma = R.get_smooth_sigma(cfg, 1000) / cfg.vox_size
    proj, _ = R.pointcloud_project_exact(cfg, points, pred["poses"], sigma)
    loss, winner = R.silhouette_loss(proj, masks, K)
    hand = (loss.double() + student_loss(pred["poses"], pred["pose_student"], winner, K, cfg.pose_predictor_student_loss_weight))
    hand = hand * cfg.proj_weight
    assert torch.equal(out["projs"], proj) and torch.equal(out["min_loss"], winner)
    assert torch.equal(total, hand)
    total.backward()
    grads = [p.grad.clone() for p in step.nets.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads) and any(float(x.abs().max()) > 0 for x in grads)


def test_train_step_without_pc_fast_with_point_dropout():
    """The branch a training run takes: points replicated per cloud, then every cloud drops its own points on the device."""
    from dpc.harness import TrainStep

    cfg = _step_cfg(pc_point_dropout=0.5, pc_point_dropout_scheduled=False)
    torch.manual_seed(7)
    step = TrainStep(cfg, "cuda", device_dropout=True)
    g = torch.Generator().manual_seed(8)
    images = torch.rand(2, 3, 32, 32, generator=g).cuda()
    masks = (torch.rand(2, 1, 32, 32, generator=g) > 0.5).float().cuda()
    total, out = step.loss(images, masks, global_step=0)
    assert out["projs"].shape == (4, 16, 16, 1) and torch.isfinite(total)
    # half of the 96 points are kept: less mass than the full clouds project, under the same networks and poses
    full, full_out = TrainStep.loss(_with_cfg(step, _step_cfg()), images, masks, global_step=0)
    assert float(out["projs"].sum()) < float(full_out["projs"].sum())
    total.backward()
    grads = [p.grad for p in step.nets.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
    loss = step(images, masks)     # zero_grad, forward, backward, Adam
    assert torch.isfinite(loss) and step.global_step == 1


def _with_cfg(step, cfg):
    """The same networks under another config (a shallow copy of the step object)."""
    import copy

    other = copy.copy(step)
    other.cfg = cfg
    return other


def test_train_step_without_pc_fast_refuses_capture_and_supervised_losses():
    from dpc.harness import TrainStep

    images, masks = torch.rand(2, 3, 32, 32).cuda(), torch.ones(2, 1, 32, 32).cuda()
    step = TrainStep(_step_cfg(), "cuda", capturable=True)
    with pytest.raises(NotImplementedError, match="pc_fast"):
        step.capture(images, masks)
    with pytest.raises(NotImplementedError, match="pc_fast"):
        step.capture_compute(images, masks)
    for key in ("proj_depth_weight", "drc_weight"):
        sup = TrainStep(_step_cfg(**{key: 1.0, "pose_predict_num_candidates": 1}), "cuda")
        with pytest.raises(NotImplementedError, match="pc_fast"):
            sup.loss(images, masks, depths=torch.ones(2, 16, 16, 1).cuda())
