"""The two ray-consistency (DRC) losses without a GPU: the fp64 oracle of tests/drc_loss_oracle.py against the reference's own
probabilities and numpy restatements of its TF-1 loss lines (F22, tests/golden/make_golden_drc_loss.py), the C ABI's
bookkeeping and argument checks, the refusals of dpc.render.drc_loss / drc_rgb_loss, the shared colour grids, and the
training step's handling of drc_weight / drc_rgb_weight."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import drc_loss_oracle as DR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpc_render.h")
NEW_SYMBOLS = ("dpc_drc_workspace_bytes", "dpc_drc_loss_fwd", "dpc_drc_loss_bwd", "dpc_drc_rgb_loss_fwd", "dpc_drc_rgb_loss_bwd")


def f22():
    return dict(np.load(os.path.join(GOLDEN, "f22_drc_loss.npz")))


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("i", [0, 1])
def test_oracle_reproduces_the_reference(i):
    """Probabilities of the reference's drc_projection and the numpy restatement of its TF-1 loss lines, to 1e-12.
    Case 1 (6 x 6 x 10) is for the math only: it reaches the oracle directly, past dpc.render's vox_size_z refusal."""
    g = f22()
    vox, colour = torch.from_numpy(g["vox%d" % i]), torch.from_numpy(g["colour%d" % i]).permute(0, 4, 1, 2, 3)
    div = torch.from_numpy(g["div%d" % i]) if "div%d" % i in g else None
    masks, images, f = torch.from_numpy(g["masks%d" % i]), torch.from_numpy(g["images%d" % i]), int(g["factor%d" % i])
    eps, div_eps, clip_after = float(g["eps%d" % i]), float(g["div_eps%d" % i]), bool(g["clip_after%d" % i])
    p = torch.flip(DR.probabilities(vox, eps), [2]).permute(1, 0, 2, 3)
    assert float((p - torch.from_numpy(g["probs%d" % i])).abs().max()) <= 1e-12
    for got, ref, what in ((DR.mask_loss(vox, None, None, masks, f, None, eps), g["loss_mask%d" % i], "mask loss"),
                           (DR.rgb_loss(vox, colour, div, images, f, None, eps, div_eps, clip_after), g["loss_rgb%d" % i], "colour loss")):
        err = abs(got.item() - float(ref))
        assert err <= 1e-12 * max(1.0, abs(float(ref))), (what, err)
    # the fixture reaches what it is meant to
    assert int(g["factor0"]) == 2 and "div0" in g and bool(g["clip_after1"]) and "div1" not in g
    assert g["vox1"].shape[1:] == (10, 6, 6) and set(np.unique(g["masks%d" % i])) == {0.0, 0.5, 1.0}
    if clip_after:
        assert float(colour.max()) > 1.0   # the after-clip acts


def test_sum_of_the_voxel_probabilities_is_not_one_minus_the_background():
    """With the e^eps factors the probabilities do not add up to one: shortening sum_{k<D} p_k to 1 - p_D errs by the size
    of the parity tolerance, which is why the kernels add the terms up."""
    g = torch.Generator().manual_seed(5)
    y = torch.rand(1, 16, 4, 4, generator=g, dtype=torch.float64) * (torch.rand(1, 16, 4, 4, generator=g) < 0.3)
    p = DR.probabilities(y, 1e-5)
    gap = (p[:, :-1].sum(1) - (1.0 - p[:, -1])).abs().max().item()
    assert 1e-6 < gap < 1e-4


def test_weights_and_sampling_rule():
    """w_s^2 per sample, / S, no 1/2; the ground truth is read at (f*y, f*x)."""
    p = torch.zeros(2, 3, 2, 2, dtype=torch.float64)
    p[:, 0], p[:, 2] = 0.25, 0.75
    masks = torch.zeros(2, 4, 4, dtype=torch.float64)
    masks[1, ::2, ::2] = 1.0            # sample 1: every sampled pixel is foreground; its other pixels stay 0
    assert DR.mask_loss_of_probabilities(p, masks, 2).item() == (4 * 0.25 + 4 * 0.75) / 2
    w = torch.tensor([3.0, 0.0], dtype=torch.float64)
    assert DR.mask_loss_of_probabilities(p, masks, 2, w).item() == 9.0 * 4 * 0.25 / 2
    vrgb = torch.zeros(2, 2, 2, 2, 3, dtype=torch.float64)
    images = torch.ones(2, 2, 2, 3, dtype=torch.float64)   # white: the background costs nothing, a black voxel 3
    assert DR.rgb_loss_of_probabilities(p, vrgb, images, 1).item() == (2 * 4 * 0.25 * 3.0) / 2


# ------------------------------------------------------------------------------------------------ 2. C ABI
def test_header_and_binding_agree_on_the_new_symbols():
    from dpc.render import _native

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(dpc_drc_\w+)\s*\(([^;]*?)\)\s*;", text)}
    protos = {k: v for k, v in protos.items() if k not in ("dpc_drc_fwd", "dpc_drc_bwd")}   # the stage-level pair, older
    assert sorted(protos) == sorted(NEW_SYMBOLS)
    L = _native.lib()
    assert L.dpc_abi_version() == 15 and _native.ABI_VERSION == 15
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    for name in NEW_SYMBOLS:
        assert name in _native.SYMBOLS
        ret, args = protos[name]
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int)
        want = []
        for a in (x.strip() for x in args.split(",")):
            if a.startswith("const DpcParams*"):
                want.append(ctypes.POINTER(_native.DpcParams))
            elif "*" in a:
                want.append(ctypes.c_void_p)
            else:
                want.append(ctype[a.split()[0]])
        assert list(fn.argtypes) == want, name


def test_argument_checks_come_before_any_launch():
    """Every refusal of the four entry points, called without a device: they return before anything is enqueued."""
    from dpc.render import _native

    L = _native.lib()
    P = _native.DpcParams(2, 0, 32, 16, 16, 0, 0, 2.0, 1.875, 1e-5, 10.0, 1, 0, None, None, None, None, None)
    ref = ctypes.byref(P)
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    SHAPE, NULL, TAPS = _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, _native.DPC_ERR_TAPS
    mf, mb, cf, cb = L.dpc_drc_loss_fwd, L.dpc_drc_loss_bwd, L.dpc_drc_rgb_loss_fwd, L.dpc_drc_rgb_loss_bwd
    # mask loss: (p, grid_wh, s, kern_z, gt, f, weights, loss_tiles, loss, stream) / (..., weights, dloss, dgrid, ds, ws, stream)
    assert mf(ref, one, None, None, one, 0, None, one, one, None) == SHAPE            # f < 1
    assert mf(ref, one, None, None, one, 65, None, one, one, None) == SHAPE           # f * H > 1024
    assert mf(ref, one, None, None, one, 1, None, one, None, None) == SHAPE           # gt without loss
    assert mf(ref, one, None, None, one, 1, None, None, one, None) == SHAPE           # ... without tiles
    assert mf(ref, None, None, None, one, 1, None, one, one, None) == NULL            # no grid
    assert mf(ref, one, None, None, None, 1, None, one, one, None) == NULL            # no gt
    assert mf(None, one, None, None, one, 1, None, one, one, None) == NULL
    assert mb(ref, one, None, None, one, 0, None, None, one, None, one, None) == SHAPE
    assert mb(ref, one, None, None, one, 65, None, None, one, None, one, None) == SHAPE
    assert mb(ref, None, None, None, one, 1, None, None, one, None, one, None) == NULL
    assert mb(ref, one, None, None, None, 1, None, None, one, None, one, None) == NULL   # no gt
    assert mb(ref, one, None, None, one, 1, None, None, None, None, one, None) == NULL   # no dgrid_wh
    assert mb(ref, one, None, None, one, 1, None, None, one, None, None, None) == NULL   # no workspace
    assert mb(None, one, None, None, one, 1, None, None, one, None, one, None) == NULL
    # colour loss: (p, vox, C, div, div_eps, clip_after, gt, f, planar, weights, loss_tiles, loss, stream) /
    #              (..., weights, dloss, dvox, dC, stream)
    assert cf(ref, one, one, None, 0.01, 0, one, 0, 0, None, one, one, None) == SHAPE
    assert cf(ref, one, one, None, 0.01, 0, one, 65, 0, None, one, one, None) == SHAPE
    assert cf(ref, one, one, None, 0.01, 0, one, 1, 0, None, one, None, None) == SHAPE    # gt without loss
    assert cf(ref, one, one, None, 0.01, 0, one, 1, 1, None, None, one, None) == SHAPE    # ... without tiles
    assert cf(ref, None, one, None, 0.01, 0, one, 1, 0, None, one, one, None) == NULL
    assert cf(ref, one, None, None, 0.01, 0, one, 1, 0, None, one, one, None) == NULL
    assert cf(ref, one, one, None, 0.01, 0, None, 1, 0, None, one, one, None) == NULL     # no gt
    assert cf(None, one, one, None, 0.01, 0, one, 1, 0, None, one, one, None) == NULL
    assert cb(ref, one, one, None, 0.01, 0, one, 0, 0, None, None, one, one, None) == SHAPE
    assert cb(ref, one, one, None, 0.01, 0, None, 1, 0, None, None, one, one, None) == NULL   # no gt
    assert cb(ref, one, one, None, 0.01, 0, one, 1, 0, None, None, None, one, None) == NULL   # no dvox
    assert cb(ref, one, one, None, 0.01, 0, one, 1, 0, None, None, one, None, None) == NULL   # no dC
    assert cb(None, one, one, None, 0.01, 0, one, 1, 0, None, None, one, one, None) == NULL
    # the colour node is stage-level: one row of points and colours per cloud
    P.point_replicas = 2
    assert cf(ref, one, one, None, 0.01, 0, one, 1, 0, None, one, one, None) == SHAPE
    assert cb(ref, one, one, None, 0.01, 0, one, 1, 0, None, None, one, one, None) == SHAPE
    P.point_replicas, P.D = 1, 2000
    assert mf(ref, one, None, None, one, 1, None, one, one, None) == SHAPE
    assert cf(ref, one, one, None, 0.01, 0, one, 1, 0, None, one, one, None) == SHAPE
    P.D, P.taps_z = 32, 4
    assert mf(ref, one, None, one, one, 1, None, one, one, None) == TAPS                  # an even kernel length
    P.taps_z = 5
    assert mf(ref, one, None, None, one, 1, None, one, one, None) == NULL                 # taps without their values
    # workspace: tickets and ds partials; a grid more for the depths and kernel lengths the generic backward serves --
    # the sizes of the depth loss's, whose buffer dpc.render shares
    P.taps_z = 0
    small = L.dpc_drc_workspace_bytes(ref)
    assert 0 < small <= 4096 and small == L.dpc_depth_workspace_bytes(ref)
    P24 = _native.DpcParams(2, 0, 24, 16, 16, 0, 0, 2.0, 1.875, 1e-5, 10.0, 1, 0, None, None, None, None, None)
    assert L.dpc_drc_workspace_bytes(ctypes.byref(P24)) >= small + 2 * 24 * 16 * 16 * 4
    P.taps_z = 33
    assert L.dpc_drc_workspace_bytes(ref) >= small + 2 * 32 * 16 * 16 * 4
    assert L.dpc_drc_workspace_bytes(None) == 0


# ------------------------------------------------------------------------------------------------ 3. dpc.render
def _outputs(S=2, G=8, **lazy):
    import dpc.render as R

    entries = {"tr_pc": torch.zeros(S, 5, 3), "voxels": torch.zeros(S, G, G, G, 1)}
    entries.update(lazy)
    return R.ProjectionOutputs(torch.zeros(S, G, G, 1), lambda: entries)


def test_refusals_name_their_key():
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    cfg = chair_unsupervised(vox_size=8)
    out, rgb, masks, images = _outputs(), torch.zeros(2, 5, 3), torch.zeros(2, 1, 8, 8), torch.zeros(2, 8, 8, 3)
    assert {"drc_loss", "drc_rgb_loss", "rgb_grids"} <= set(R.__all__)
    with pytest.raises(NotImplementedError, match="pose_predict_num_candidates"):
        R.drc_loss(cfg, _outputs(S=8), masks)
    with pytest.raises(NotImplementedError, match="pose_predict_num_candidates"):
        R.drc_rgb_loss(cfg, _outputs(S=8), torch.zeros(8, 5, 3), images)
    cfg_z = chair_unsupervised(vox_size=8, vox_size_z=10)
    with pytest.raises(NotImplementedError, match="vox_size_z"):
        R.drc_loss(cfg_z, out, masks)
    with pytest.raises(NotImplementedError, match="vox_size_z"):
        R.drc_rgb_loss(cfg_z, out, rgb, images)
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt"):
        R.drc_loss(chair_unsupervised(vox_size=8, pc_gauss_filter_gt=True), out, masks)
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt_rgb"):
        R.drc_rgb_loss(chair_unsupervised(vox_size=8, pc_gauss_filter_gt_rgb=True), out, rgb, images)
    with pytest.raises(ValueError, match="integer multiple"):
        R.drc_loss(cfg, out, torch.zeros(2, 12, 12, 1))
    with pytest.raises(ValueError, match="masks must be"):
        R.drc_loss(cfg, out, torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match="integer multiple"):
        R.drc_rgb_loss(cfg, out, rgb, torch.zeros(2, 3, 16, 8))
    with pytest.raises(ValueError, match="all_rgb must hold"):
        R.drc_rgb_loss(cfg, out, torch.zeros(2, 4, 3), images)
    for fn, args in ((R.drc_loss, (masks,)), (R.drc_rgb_loss, (rgb, images)), (R.rgb_grids, (rgb,))):
        with pytest.raises(TypeError, match="pointcloud_project_fast"):
            fn(cfg, {"proj": out["proj"]}, *args)
    # vox_size_z equal to vox_size is a cubic grid: not refused (the next check speaks)
    with pytest.raises(ValueError, match="integer multiple"):
        R.drc_loss(chair_unsupervised(vox_size=8, vox_size_z=8), out, torch.zeros(2, 12, 12, 1))


@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhw"])
def test_staged_outputs_take_the_torch_route(layout):
    """Outputs that did not come from the fused path (a Gaussian beyond its window): the same numbers from drc_probs."""
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    g = torch.Generator().manual_seed(3)
    probs = torch.rand(5, 2, 4, 4, 1, generator=g, dtype=torch.float64)
    masks = (torch.rand(2, 8, 8, generator=g) < 0.5).double()
    w = torch.tensor([0.5, 2.0], dtype=torch.float64)
    out = _outputs(G=4, drc_probs=probs)
    shaped = {"nchw": masks.unsqueeze(1), "nhwc": masks.unsqueeze(-1), "nhw": masks}[layout]
    got = R.drc_loss(chair_unsupervised(vox_size=4), out, shaped, w)
    ref = DR.mask_loss_of_probabilities(probs[..., 0].permute(1, 0, 2, 3), masks, 2, w)
    assert abs(got.item() - ref.item()) <= 1e-13 * ref.item()


def test_the_three_colour_functions_accept_shared_grids(monkeypatch):
    """grids= (what rgb_grids returned) reaches the nodes in place of grids made on the spot; None is today's behaviour."""
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    cfg = chair_unsupervised(vox_size=8, pc_rgb_divide_by_occupancies=True)
    out, rgb, images = _outputs(), torch.zeros(2, 5, 3), torch.zeros(2, 16, 16, 3)
    made = []
    sentinel = ("geom", torch.zeros(2, 8, 8, 8), torch.zeros(2, 3, 8, 8, 8), torch.ones(2, 8, 8, 8))

    def fake_grids(cfg_, outputs, all_rgb, kernel, point_index=None):
        made.append((outputs, all_rgb, kernel))
        return sentinel

    seen = {}

    def node(name, ret):
        class Node:
            @staticmethod
            def apply(vox, C, div, *rest):
                seen[name] = (vox, C, div) + rest
                return ret
        return Node

    monkeypatch.setattr(R, "_rgb_grids", fake_grids)
    monkeypatch.setattr(R, "RgbLoss", node("proj", (torch.zeros(()), torch.zeros(2, 8, 8, 3))))
    monkeypatch.setattr(R, "RgbMap", node("map", torch.zeros(2, 8, 8, 3)))
    monkeypatch.setattr(R, "DrcRgbLoss", node("drc", torch.zeros(())))
    grids = R.rgb_grids(cfg, out, rgb, "kernel")
    assert grids is sentinel and made == [(out, rgb, "kernel")]
    R.proj_rgb_loss(cfg, out, rgb, images, "kernel", grids=grids)
    R.drc_rgb_loss(cfg, out, rgb, images, "kernel", grids=grids)
    R.project_rgb(cfg, out, rgb, "kernel", grids=grids)
    assert len(made) == 1                                   # one splat and one smoothing for all three
    for name in ("proj", "map", "drc"):
        assert all(a is b for a, b in zip(seen[name][:3], sentinel[1:])), name
    assert seen["drc"][3:] == (images, 2, False, None, "geom", 0.01, False) == seen["proj"][3:]
    R.proj_rgb_loss(cfg, out, rgb, images, "kernel")
    R.drc_rgb_loss(cfg, out, rgb, images, "kernel")
    R.project_rgb(cfg, out, rgb, "kernel")
    assert len(made) == 4                                   # grids=None: each makes its own, as before


# ------------------------------------------------------------------------------------------------ 4. the training step
def _step(**kw):
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.step import TrainStep

    cfg = chair_unsupervised(batch_size=1, step_size=2, vox_size=32, pc_num_points=64, pose_predictor_student=False,
                             pc_point_dropout=1.0, pc_relative_sigma=1.0, pc_relative_sigma_end=1.0, input_shape=[64, 64, 3], **kw)
    torch.manual_seed(0)
    return cfg, TrainStep(cfg, torch.device("cpu"))


def test_train_step_picks_up_the_drc_weights(monkeypatch):
    """drc_weight / drc_rgb_weight reach the total through dpc.render.drc_loss / drc_rgb_loss on the projection of the step,
    with the pooled masks at f = 1 and colour grids shared with proj_rgb_loss; with both weights 0 nothing changes.
    The renderer is replaced by stand-ins: this runs without a device."""
    import dpc.harness.step as S
    import dpc.render as R

    calls = []

    def project(cfg, pc, q, t, rgb, kernel, **kw):
        calls.append("project")
        proj = pc.sum().reshape(1, 1, 1, 1).expand(q.shape[0], 32, 32, 1) * 0.0
        return R.ProjectionOutputs(proj, lambda: {})

    def silhouette(pred, gt, K, w=None):
        return pred.sum() + 1.0, torch.zeros(pred.shape[0], dtype=torch.int32)

    def drc(cfg, outputs, masks, w=None):
        calls.append(("drc", tuple(masks.shape), masks))
        return outputs["proj"].sum() + 3.0

    def grids(cfg, outputs, all_rgb, kernel=None):
        calls.append("grids")
        return "shared"

    def proj_rgb(cfg, outputs, all_rgb, images, kernel=None, w=None, return_rgb=False, grids=None):
        calls.append(("proj_rgb", grids))
        return all_rgb.sum() * 0.0 + 5.0, None

    def drc_rgb(cfg, outputs, all_rgb, images, kernel=None, w=None, grids=None):
        calls.append(("drc_rgb", grids))
        return all_rgb.sum() * 0.0 + 7.0

    def unsupervised(*a, **kw):
        raise RuntimeError("the one-call step")

    for name, fn in (("pointcloud_project_fast", project), ("silhouette_loss", silhouette), ("drc_loss", drc), ("rgb_grids", grids),
                     ("proj_rgb_loss", proj_rgb), ("drc_rgb_loss", drc_rgb), ("pointcloud_project_loss", unsupervised)):
        monkeypatch.setattr(S.R, name, fn)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 64, 64, generator=g)
    masks = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float()

    cfg, step = _step(pose_predict_num_candidates=1, drc_weight=0.5)
    total, out = step.loss(images, masks)
    assert abs(total.item() - (1.0 * 1.0 + 0.5 * 3.0)) < 1e-12 and out["drc_loss"].item() == 3.0
    (_, shape, pooled), = [c for c in calls if c[0] == "drc"]
    assert shape == (2, 32, 32, 1) and torch.equal(pooled, S.pooled_masks(masks, 32)) and "grids" not in calls
    with pytest.raises(NotImplementedError, match="drc_weight"):
        step.capture(images, masks)
    with pytest.raises(NotImplementedError, match="drc_weight"):
        step.capture_compute(images, masks)

    calls.clear()
    cfg, step = _step(pose_predict_num_candidates=1, pc_rgb=True, proj_rgb_weight=2.0, drc_rgb_weight=0.25)
    total, out = step.loss(images, masks)
    assert abs(total.item() - (1.0 + 2.0 * 5.0 + 0.25 * 7.0)) < 1e-12 and out["drc_rgb_loss"].item() == 7.0
    assert calls.count("grids") == 1 and ("proj_rgb", "shared") in calls and ("drc_rgb", "shared") in calls
    with pytest.raises(NotImplementedError, match="rgb_weight"):
        step.capture(images, masks)
    calls.clear()
    cfg, step = _step(pose_predict_num_candidates=1, pc_rgb=True, drc_rgb_weight=0.25)   # the drc colour term alone
    total, out = step.loss(images, masks)
    assert abs(total.item() - (1.0 + 0.25 * 7.0)) < 1e-12 and "rgb_loss" not in out
    with pytest.raises(NotImplementedError, match="drc_rgb_weight"):
        step.capture(images, masks)
    cfg, step = _step(pose_predict_num_candidates=1, drc_rgb_weight=0.25)                # without pc_rgb the key is not read
    with pytest.raises(RuntimeError, match="the one-call step"):
        step.loss(images, masks)

    # both terms need one pose candidate per image
    for kw in (dict(drc_weight=0.5), dict(pc_rgb=True, drc_rgb_weight=0.5)):
        cfg, step = _step(pose_predict_num_candidates=4, **kw)
        with pytest.raises(NotImplementedError, match="pose_predict_num_candidates"):
            step.loss(images, masks)
    # with both weights 0 the step is the one it was
    cfg, step = _step(pose_predict_num_candidates=1)
    assert cfg.drc_weight == 0.0 and cfg.drc_rgb_weight == 0.0
    with pytest.raises(RuntimeError, match="the one-call step"):
        step.loss(images, masks)
