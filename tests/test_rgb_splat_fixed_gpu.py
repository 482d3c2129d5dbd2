"""The bit-reproducible colour splat on the GPU (csrc/dpc_rgb_splat.hip, cfg.pc_rgb_deterministic) against the fp64 oracle of
tests/rgb_oracle.py, and against itself: bit for bit under a permutation of the points, from call to call, and between
colour sets read in place and the replicated tensor.

Comparisons with the oracle use the parity rule of tests/test_gpu_parity.py, max |device - reference| <= 1e-5 * max(1, max
|reference|), behind rgb_oracle.clip_margin's guard (no value near a clip threshold; the seeds were checked on the CPU).
Inputs are made like node_inputs of tests/test_rgb_loss_gpu.py -- they ARE that function's, at this file's shapes:
    A  3 clouds, 12 x 20 x 20, 300 points (a blob one cell wide, a twentieth outside the cube, one coordinate at exactly
       -1/2, one just under +1/2);
    B  4 clouds on 2 colour sets of 300 colours, 200 points each through a point_index drawn without replacement, same grid;
    C  2 clouds, 8^3, 4096 points inside ONE cell, colours 0.95: a voxel takes thousands of adds and sums far above 1."""
import numpy as np
import pytest
import torch

import drc_loss_oracle as DL
import rgb_oracle as RO
from oracle import dpc_oracle as O
from test_rgb_loss_gpu import COLOUR_MARGIN, DRC_MARGIN, EPS, Case, assert_margins, close, dev, fake_outputs, node_inputs

pytestmark = pytest.mark.gpu

DET = dict(pc_rgb_deterministic=True)
A_CASES = [
    Case("a_taps5", 3, 12, 20, 300, 5, 1.6, f=2, weights=True, seed=21, **DET),
    Case("a_notaps", 3, 12, 20, 300, 0, 0.0, planar=True, seed=22, **DET),
    Case("a_divide", 3, 12, 20, 300, 5, 1.6, seed=23, pc_rgb_divide_by_occupancies=True, **DET),
]
# drc_rgb_loss takes cubic grids only (it refuses vox_size_z != vox_size, as the reference's ray potentials do not broadcast
# there), so its case is shape A with the sides cut to the depth: 12 x 12 x 12, nothing larger than A
A_CUBE = Case("a_cube12", 3, 12, 12, 300, 5, 1.6, f=2, weights=True, seed=25, **DET)
B_CASE = Case("b_sets", 4, 12, 20, 200, 5, 1.6, weights=True, seed=24, **DET)
N_SET = 300


def images_of(c, images):
    return (images.permute(0, 3, 1, 2).contiguous() if c.planar else images).cuda()


def c_inputs():
    """Shape C: every point of a cloud inside one cell (fractions in [0.05, 0.95]), colours 0.95, sparse occupancies."""
    g = torch.Generator().manual_seed(7100)
    B, G, N = 2, 8, 4096
    cell = torch.tensor([[2.0, 3.0, 4.0], [5.0, 1.0, 2.0]]).unsqueeze(1)
    tr = ((cell + 0.05 + 0.9 * torch.rand(B, N, 3, generator=g)) / (G - 1.0) - 0.5).float()
    rgb = torch.full((B, N, 3), 0.95)
    vox = (torch.rand(B, G, G, G, generator=g) * (torch.rand(B, G, G, G, generator=g) < 0.4)).float()
    images = torch.rand(B, G, G, 3, generator=g)
    return tr, rgb, vox, images


C_CFG = O.Cfg(vox_size=8, pc_gauss_kernel_size=3, drc_logsum_clip_val=EPS, **DET)
_REF = {}


def a_reference(c):
    """Oracle results of a shape-A case (raw grid, image, colour volume, loss, gradients), computed once and shared."""
    if c.name not in _REF:
        tr, rgb, vox, images, w, _ = node_inputs(c)
        cfg, kern = c.cfg(), c.kernel(O)
        assert_margins(c, cfg, kern, tr, rgb, vox)
        leaves = [x.double().requires_grad_(True) for x in (tr, rgb, vox)]
        parts = {}
        proj, vrgb, loss = RO.rgb_loss(cfg, *leaves, kern, images, c.f, w, parts=parts)
        loss.backward()
        _REF[c.name] = dict(raw=parts["raw"].detach(), proj=proj.detach(), vrgb=vrgb.detach(), loss=loss.detach(),
                            grads=[x.grad for x in leaves], inside=((tr >= -0.5) & (tr <= 0.5)).all(-1))
    return _REF[c.name]


def run(cfg, kern, tr, rgb, vox, images, w=None, f=1, point_index=None, backward=True):
    """The deterministic route on device leaves: dict of the raw grid, the loss and the gradients."""
    import dpc.render as R
    from dpc.render._ops import RgbSplatFixed

    leaves = [dev(x, True) for x in (tr, rgb, vox)]
    idx = None if point_index is None else point_index.cuda()
    out = fake_outputs(leaves[0], leaves[2])
    with torch.no_grad():
        raw = RgbSplatFixed.apply(leaves[0], leaves[1], R._geometry(cfg, kern), False, idx)
    loss = R.proj_rgb_loss(cfg, out, leaves[1], images, kern, None if w is None else w.cuda(), point_index=idx)
    if backward:
        loss.backward()
    return dict(raw=raw, loss=loss.detach(), dtr=leaves[0].grad, drgb=leaves[1].grad, dvox=leaves[2].grad)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("c", A_CASES, ids=repr)
def test_parity(c):
    import dpc.render as R
    from dpc.render._ops import RgbSplatFixed

    ref = a_reference(c)
    tr, rgb, vox, images, w, _ = node_inputs(c)
    cfg, kern = c.cfg(), c.kernel(R)
    leaves = [dev(x, True) for x in (tr, rgb, vox)]
    out = fake_outputs(leaves[0], leaves[2])
    wd = None if w is None else w.cuda()
    with torch.no_grad():
        raw = RgbSplatFixed.apply(leaves[0], leaves[1], R._geometry(cfg, kern), False)
    close(raw, ref["raw"], what=c.name + " raw colour grid")
    loss, proj = R.proj_rgb_loss(cfg, out, leaves[1], images_of(c, images), kern, wd, return_rgb=True)
    maps = R.project_rgb(cfg, out, leaves[1], kern)
    close(loss, ref["loss"], what=c.name + " loss")
    close(proj, ref["proj"], what=c.name + " proj_rgb (loss launch)")
    close(maps["proj_rgb"], ref["proj"], what=c.name + " proj_rgb")
    close(maps["voxels_rgb"], ref["vrgb"], what=c.name + " voxels_rgb")
    loss.backward()
    for name, x, r in zip(("d(tr)", "d(rgb)", "d(vox)"), leaves, ref["grads"]):
        close(x.grad, r, what="%s %s" % (c.name, name))
        assert float(r.abs().max()) > 1e-4
    outside = ~ref["inside"].cuda()
    assert not leaves[1].grad[outside].any() and not leaves[0].grad[outside].any()


# ------------------------------------------------------------------------------------------------ 2. order independence
def _permuted(tr, rgb, seed):
    g = torch.Generator().manual_seed(seed)
    perm = torch.stack([torch.randperm(tr.shape[1], generator=g) for _ in range(tr.shape[0])])
    take = perm.unsqueeze(-1).expand(-1, -1, 3)
    return perm, tr.gather(1, take), rgb.gather(1, take)


def _assert_order_independent(cfg, kern, tr, rgb, vox, images, w, f, live_gradients):
    a = run(cfg, kern, tr, rgb, vox, images, w, f)
    again = run(cfg, kern, tr, rgb, vox, images, w, f)
    perm, tr_p, rgb_p = _permuted(tr, rgb, 99)
    assert not perm.equal(torch.arange(tr.shape[1]).expand_as(perm))
    p = run(cfg, kern, tr_p, rgb_p, vox, images, w, f)
    take = perm.cuda().unsqueeze(-1).expand(-1, -1, 3)
    assert float(a["raw"].abs().max()) > 1.0 and torch.isfinite(a["loss"])
    for other, what in ((again, "a second call"), (p, "permuted points")):
        assert torch.equal(a["raw"], other["raw"]), "colour grid: " + what
        assert torch.equal(a["loss"], other["loss"]), "loss: " + what
        assert torch.equal(a["dvox"], other["dvox"]), "d(vox): " + what
    assert torch.equal(a["dtr"], again["dtr"]) and torch.equal(a["drgb"], again["drgb"])
    # gradients of the permuted run, taken back to the original order
    assert torch.equal(a["dtr"].gather(1, take), p["dtr"]) and torch.equal(a["drgb"].gather(1, take), p["drgb"])
    # (shape C: every voxel the points touch sits far above the clip, whose backward passes nothing on to them)
    assert not live_gradients or (bool(a["drgb"].any()) and bool(a["dtr"].any()))


def test_order_independence_shape_a():
    import dpc.render as R

    c = A_CASES[0]
    tr, rgb, vox, images, w, _ = node_inputs(c)
    _assert_order_independent(c.cfg(), c.kernel(R), tr, rgb, vox, images.cuda(), w, c.f, True)


def test_order_independence_shape_c():
    tr, rgb, vox, images = c_inputs()
    _assert_order_independent(C_CFG, None, tr, rgb, vox, images.cuda(), None, 1, False)


# ------------------------------------------------------------------------------------------------ 3. no wrap
def test_no_wrap_shape_c():
    tr, rgb, vox, images = c_inputs()
    colour, drc = RO.clip_margin(C_CFG, tr, rgb, vox, None)
    assert colour > COLOUR_MARGIN and drc > DRC_MARGIN
    parts = {}
    _, _, loss = RO.rgb_loss(C_CFG, tr, rgb, vox, None, images, 1, parts=parts)
    assert float(parts["raw"].max()) > 400.0          # far above 1: thousands of adds into one voxel
    got = run(C_CFG, None, tr, rgb, vox, images.cuda(), backward=False)
    assert torch.isfinite(got["raw"]).all() and torch.isfinite(got["loss"])
    close(got["raw"], parts["raw"], what="shape C raw colour grid")
    close(got["loss"], loss, what="shape C loss")


# ------------------------------------------------------------------------------------------------ 4. sets in place
def b_inputs(with_index=True):
    c = B_CASE
    tr, _, vox, images, w, _ = node_inputs(c)
    g = torch.Generator().manual_seed(7200)
    n_set = N_SET if with_index else c.N
    sets = (0.05 + 0.9 * torch.rand(2, n_set, 3, generator=g)).float()
    index = torch.stack([torch.randperm(N_SET, generator=g)[:c.N] for _ in range(c.B)]).to(torch.int32) if with_index else None
    return tr, sets, index, vox, images, w


@pytest.mark.parametrize("with_index", [True, False], ids=["point_index", "no_index"])
def test_sets_in_place(with_index):
    import dpc.render as R

    c = B_CASE
    cfg, kern = c.cfg(), c.kernel(R)
    tr, sets, index, vox, images, w = b_inputs(with_index)
    img = images.cuda()
    s1 = run(cfg, kern, tr, sets, vox, img, w, c.f, point_index=index)
    s2 = run(cfg, kern, tr, sets, vox, img, w, c.f, point_index=index)
    # the replicated tensor through the same deterministic route; its gradient goes back to the sets through autograd
    leaf = dev(sets, True)
    rep = R.replicate_rgb(leaf, c.B, None if index is None else index.cuda())
    assert rep.shape == tr.shape
    tr_d, vox_d = dev(tr, True), dev(vox, True)
    loss = R.proj_rgb_loss(cfg, fake_outputs(tr_d, vox_d), rep, img, kern, w.cuda())
    loss.backward()
    r = run(cfg, kern, tr, rep.detach().cpu(), vox, img, w, c.f, backward=False)
    assert torch.equal(s1["raw"], r["raw"]) and torch.equal(s1["loss"], loss.detach()) and float(s1["raw"].abs().max()) > 1.0
    assert torch.equal(s1["dtr"], tr_d.grad) and torch.equal(s1["dvox"], vox_d.grad)
    assert s1["drgb"].shape == sets.shape and float(leaf.grad.abs().max()) > 1e-4
    close(s1["drgb"], leaf.grad.double(), what="d(colour sets) against autograd through replicate_rgb")
    assert torch.equal(s1["drgb"], s2["drgb"]) and torch.equal(s1["loss"], s2["loss"])
    # clouds 0 and 1 (both on set 0) swap all their inputs: the same integer contributions arrive in another order
    swap = torch.tensor([1, 0, 2, 3])
    sw = run(cfg, kern, tr[swap], sets, vox[swap], img[swap.cuda()], w[swap], c.f, point_index=None if index is None else index[swap])
    assert torch.equal(s1["drgb"], sw["drgb"])
    assert torch.equal(s1["dtr"][swap.cuda()], sw["dtr"])


# ------------------------------------------------------------------------------------------------ 5. range guard
def test_range_guard_colours():
    import dpc.render as R

    c = A_CASES[1]
    cfg = c.cfg()
    tr, rgb, vox, images, w, _ = node_inputs(c)
    inside = ((tr >= -0.5) & (tr <= 0.5)).all(-1)
    j = int(torch.nonzero(inside[1])[0])
    img = images_of(c, images)
    clean = run(cfg, None, tr, rgb, vox, img, backward=False)
    assert torch.isfinite(clean["raw"]).all()
    for bad in (8.5, float("nan"), float("inf"), -float("inf")):
        x = rgb.clone()
        x[1, j, 1] = bad
        got = run(cfg, None, tr, x, vox, img, backward=False)     # returns normally
        assert torch.isnan(got["raw"][1]).all(), bad
        assert torch.equal(got["raw"][0], clean["raw"][0]) and torch.equal(got["raw"][2], clean["raw"][2]), bad
    # exactly 8 is inside the range: accepted, and the oracle's value
    x = rgb.clone()
    x[1, j, 1] = 8.0
    x[0, j, 0] = -8.0
    got = run(cfg, None, tr, x, vox, img, backward=False)
    close(got["raw"], RO.splat_rgb(cfg, tr, x), what="colours of exactly +-8")


def test_range_guard_set_gradients():
    """A gradient contribution beyond grad_fits_fixed (2^20) turns the gradient of ITS colour set into NaN, and no other."""
    import dpc.render as R
    from dpc.render._ops import RgbSplatFixed

    c = B_CASE
    tr, sets, index, _, _, _ = b_inputs()
    geom = R._geometry(c.cfg(), None)

    def drgb(scale0):
        leaf = dev(sets, True)
        C = RgbSplatFixed.apply(tr.cuda(), leaf, geom, True, index.cuda())
        dC = torch.ones_like(C)
        dC[0] *= scale0        # cloud 0 reads set 0
        C.backward(dC)
        return leaf.grad

    clean, hot = drgb(1.0), drgb(4.0e6)     # sum_corners w * 4e6 = 4e6 > 2^20 for every point inside the grid
    assert torch.isfinite(clean).all() and bool(clean[0].any()) and bool(clean[1].any())
    assert torch.isnan(hot[0]).all()
    assert torch.equal(hot[1], clean[1])


# ------------------------------------------------------------------------------------------------ 6. the two backwards
def test_backward_bits_equal_the_default_route():
    """Per-cloud colours (no sets, no point_index): both routes' backward is a pure gather through one body, so d(tr) and
    d(rgb) of RgbSplat and RgbSplatFixed are the same bits, with and without stop_points_gradient."""
    import dpc.render as R
    from dpc.render._ops import RgbSplat, RgbSplatFixed

    c = A_CUBE
    tr, rgb, _, _, _, _ = node_inputs(c)
    geom = R._geometry(c.cfg(), None)
    dC = torch.randn(c.B, 3, c.D, c.G, c.G, generator=torch.Generator().manual_seed(7300)).cuda()
    for stop in (False, True):
        grads = []
        for node in (RgbSplat, RgbSplatFixed):
            leaves = [dev(tr, True), dev(rgb, True)]
            node.apply(leaves[0], leaves[1], geom, stop).backward(dC)
            grads.append([x.grad for x in leaves])
        (dtr, drgb), (dtr_fixed, drgb_fixed) = grads
        assert torch.equal(drgb, drgb_fixed) and float(drgb.abs().max()) > 1e-3, stop
        if stop:
            assert dtr is None and dtr_fixed is None
        else:
            assert torch.equal(dtr, dtr_fixed) and float(dtr.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 7. drc_rgb_loss
def test_drc_rgb_loss_through_shared_grids():
    import dpc.render as R

    c = A_CUBE
    ref = a_reference(c)      # checks the margins
    tr, rgb, vox, images, w, _ = node_inputs(c)
    cfg, kern = c.cfg(), c.kernel(R)
    with torch.no_grad():
        C = RO.colour_grid(cfg, tr, rgb, c.kernel(O))
    want = DL.rgb_loss(vox.double(), C, None, images, c.f, w, eps=EPS)
    img, wd = images.cuda(), w.cuda()
    losses = []
    for _ in range(2):
        out = fake_outputs(tr.cuda(), vox.cuda())
        grids = R.rgb_grids(cfg, out, rgb.cuda(), kern)
        losses.append(R.drc_rgb_loss(cfg, out, rgb.cuda(), img, kern, wd, grids=grids))
        shared = R.proj_rgb_loss(cfg, out, rgb.cuda(), img, kern, wd, grids=grids)
    close(losses[0], want, what="drc_rgb_loss on the deterministic grids")
    close(shared, ref["loss"], what="proj_rgb_loss on the same grids")
    assert torch.equal(losses[0], losses[1])


# ------------------------------------------------------------------------------------------------ 8. empty inputs
def test_empty_inputs():
    import dpc.render as R

    cfg = A_CASES[1].cfg()
    D, G = 12, 20
    # no clouds
    out = fake_outputs(torch.zeros(0, 5, 3, device="cuda"), torch.zeros(0, D, G, G, device="cuda"))
    rgb = torch.zeros(0, 5, 3, device="cuda", requires_grad=True)
    geom, vox, C, div = R.rgb_grids(cfg, out, rgb, None)
    assert C.shape == (0, 3, D, G, G)
    loss = R.proj_rgb_loss(cfg, out, rgb, torch.zeros(0, G, G, 3, device="cuda"), None, grids=(geom, vox, C, div))
    assert float(loss.detach()) == 0.0
    # no points: the grid is zeroed, and the loss is that of an empty colour volume
    g = torch.Generator().manual_seed(5)
    voxels, images = torch.rand(2, D, G, G, generator=g) * 0.5, torch.rand(2, G, G, 3, generator=g)
    out = fake_outputs(torch.zeros(2, 0, 3, device="cuda"), voxels.cuda())
    rgb = torch.zeros(2, 0, 3, device="cuda", requires_grad=True)
    grids = R.rgb_grids(cfg, out, rgb, None)
    assert grids[2].shape == (2, 3, D, G, G) and not grids[2].any()
    loss = R.proj_rgb_loss(cfg, out, rgb, images.cuda(), None, grids=grids)
    want = RO.loss_of_rgb(RO.integrate(cfg, torch.zeros(2, 3, D, G, G, dtype=torch.float64), voxels), images, 1)
    close(loss, want, what="loss without points")
    loss.backward()
    torch.cuda.synchronize()
    assert rgb.grad is None or rgb.grad.shape == (2, 0, 3)


# ------------------------------------------------------------------------------------------------ 9. harness
def test_harness_reads_colour_sets_in_place():
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.step import TrainStep

    kw = dict(batch_size=1, step_size=2, vox_size=16, pc_num_points=200, pose_predictor_student=False, pc_point_dropout=0.7,
              pc_relative_sigma=1.0, pc_relative_sigma_end=1.0, input_shape=[64, 64, 3], pc_rgb=True, proj_rgb_weight=1.0,
              pose_predict_num_candidates=1)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 64, 64, generator=g).cuda()
    masks = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()
    res = {}
    for key in (False, True):
        torch.manual_seed(0)
        step = TrainStep(chair_unsupervised(pc_rgb_deterministic=key, **kw), torch.device("cuda"))
        np.random.seed(11)                      # the host RNG of the point dropout: both steps drop the same points
        total, out = step.loss(images, masks)
        total.backward()
        dec = step.nets.decoder
        res[key] = (total.detach(), out, {n: p.grad for n, p in dec.named_parameters() if n.startswith("rgb_raw_dec")})
    (t0, out0, g0), (t1, out1, g1) = res[False], res[True]
    assert "all_rgb" in out0 and out0["all_rgb"].shape[0] == 2 and 100 < out0["all_rgb"].shape[1] < 200   # the kept points
    assert "all_rgb" not in out1 and out1["rgb_1"].shape == (1, 200, 3)
    assert float(out1["rgb_loss"].detach()) > 0
    close(t1, t0.double(), what="total loss, keyed against unkeyed")
    assert set(g0) == set(g1) and len(g0) == 2
    for n in g0:
        assert g0[n] is not None and bool(g0[n].any())
        close(g1[n], g0[n].double(), what="d(%s)" % n)
