"""CPU-side checks of the exact Gaussian renderer (cfg.pc_fast == false): the oracle against the stored fixture and against
itself (literal broadcast form == separable form, analytic gradient == autograd of the literal form), the C ABI's symbols,
prototypes and refusals (every one returns before a launch, so they run without a device), and the Python layer's refusals
and exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gauss_voxels_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dpc_render.h")


# ------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("mode", [GO.NONE, GO.ANALYTICAL, GO.PER_POINT])
@pytest.mark.parametrize("G,sigma_rel", [(9, 1.0), (12, 0.5), (7, 3.0)])
def test_literal_form_equals_the_separable_form(mode, G, sigma_rel):
    rng = np.random.default_rng(100 * G + mode)
    tr = GO.points(rng, 2, 21)
    sigma = sigma_rel / G
    raw_l, vox_l = GO.pointcloud2voxels_literal(tr, G, sigma, mode, chunk=5)
    raw_s = GO.raw_separable(tr, G, sigma, mode)
    # meshgrid's 'xy' indexing: the literal grid's axes follow components (1, 0, 2), the kernels' (0, 1, 2)
    assert np.abs(raw_l[..., 0] - raw_s.transpose(0, 2, 1, 3)).max() <= 1e-13 * max(1.0, raw_s.max())
    assert np.abs(raw_l[..., 0] - raw_s).max() > 1e-3 * raw_s.max(), "the case cannot tell the two axis orders apart"
    assert np.array_equal(vox_l, np.clip(raw_l, 0.0, 1.0))
    raw_t, vox_t = GO.literal_torch(torch.from_numpy(tr), G, sigma, mode)
    assert np.abs(raw_t.numpy() - raw_l).max() <= 1e-13 * max(1.0, raw_l.max())


@pytest.mark.parametrize("mode", [GO.NONE, GO.ANALYTICAL, GO.PER_POINT])
def test_analytic_gradient_equals_autograd_of_the_literal_form(mode):
    G, sigma = 9, 1.2 / 9
    rng = np.random.default_rng(7 + mode)
    tr = GO.points(rng, 2, 40)
    dvox = rng.standard_normal((2, G, G, G))          # kernel layout
    t = torch.from_numpy(tr).double().requires_grad_(True)
    raw, vox = GO.literal_torch(t, G, sigma, mode)
    (vox[..., 0] * torch.from_numpy(dvox).transpose(1, 2)).sum().backward()
    got = GO.grad_separable(tr, G, sigma, mode, dvox)
    assert (raw > 1).any() or mode != GO.NONE, "the unnormalised case should clip somewhere"
    assert np.abs(got - t.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(got).max())
    assert np.abs(got).max() > 0.1


def test_oracle_reproduces_the_fixture(golden):
    from oracle import dpc_oracle as O

    g = golden("f23_gauss_voxels.npz")
    G, sigma = g["voxels"].shape[1], float(g["sigma"])
    assert g["voxels"].shape == (2, G, G, G, 1) and g["proj"].shape == (2, G, G, 1)
    for tag, mode in (("none", GO.NONE), ("analytical", GO.ANALYTICAL), ("per_point", GO.PER_POINT)):
        raw, _ = GO.pointcloud2voxels_literal(g["tr_pc"], G, sigma, mode)
        assert np.abs(raw - g["raw_" + tag]).max() <= 1e-13 * max(1.0, g["raw_" + tag].max())
        sep = GO.raw_separable(g["tr_pc"], G, sigma, mode)
        assert np.abs(sep.transpose(0, 2, 1, 3) - g["raw_" + tag][..., 0]).max() <= 1e-13 * max(1.0, sep.max())
    # pointcloud_project transposes once more (point_cloud.py:222): its grids are in the kernels' layout
    assert np.abs(g["raw"] - g["raw_analytical"].transpose(0, 2, 1, 3, 4)).max() <= 1e-13
    assert np.array_equal(g["voxels"], np.clip(g["raw"], 0.0, 1.0))
    lo, near1 = GO.clip_margin(g["raw"])
    assert lo >= 0.0 and near1 > 1e-6 and (g["raw"] > 1).any()
    # the whole chain on the project's own torch oracle of the transform and the DRC
    cfg = O.Cfg(vox_size=G)
    pc = torch.from_numpy(g["pc"]).double().requires_grad_(True)
    q = torch.from_numpy(g["q"]).double().requires_grad_(True)
    proj, voxels, raw = GO.pointcloud_project(cfg, pc, q, sigma)
    assert np.abs(raw.detach().numpy() - g["raw"]).max() <= 1e-12
    assert np.abs(proj.detach().numpy() - g["proj"]).max() <= 1e-12
    ((voxels * torch.from_numpy(g["dvox"])).sum() + (proj * torch.from_numpy(g["dproj"])).sum()).backward()
    assert np.abs(pc.grad.numpy() - g["dpc"]).max() <= 1e-10 * np.abs(g["dpc"]).max()
    assert np.abs(q.grad.numpy() - g["dq"]).max() <= 1e-10 * np.abs(g["dq"]).max()
    # the analytic gradient of the voxel stage alone, against autograd through the stored transformed points
    t = torch.from_numpy(g["tr_pc"]).requires_grad_(True)
    _, v = GO.literal_torch(t, G, sigma, GO.ANALYTICAL)
    (v.permute(0, 2, 1, 3, 4) * torch.from_numpy(g["dvox"])).sum().backward()
    got = GO.grad_separable(g["tr_pc"], G, sigma, GO.ANALYTICAL, g["dvox"][..., 0])
    assert np.abs(got - t.grad.numpy()).max() <= 1e-12 * np.abs(got).max()


def _table_clouds(golden):
    """(tr, G, sigma) of the fixture and of the GPU file's underflow and width cases."""
    import test_gauss_voxels_gpu as TG

    g = golden("f23_gauss_voxels.npz")
    yield g["tr_pc"], int(g["voxels"].shape[1]), float(g["sigma"])
    for tag in TG.ids(TG.UNDERFLOW) + ["w1_pp", "w2_pp", "w3_pp", "w16", "w33", "t40_n2", "t24_n128", "g24_n257", "g40"]:
        _, _, G, sigma, _, tr, _ = TG.case_inputs(tag)
        yield tr, G, sigma


def test_shifted_tables_equal_the_plain_quotient_where_that_is_finite(golden):
    """Element by element to 1e-12 relative, wherever the plain form is finite and well defined: its numerator exp(arg)
    must be a normal fp64 number with digits to spare (above 1e-290); below that the plain quotient has lost digits, or is
    0 where the shifted one is not, through no fault of the shift.  dP = P (w - wbar) is a difference that cancels where a
    point's table sits on one voxel, so its scale is P max|w|, not |dP|."""
    rows = nans = 0
    for tr, G, sigma in _table_clouds(golden):
        Ps, dPs = GO.tables(tr, G, sigma, GO.PER_POINT)
        Pp, dPp = GO.tables(tr, G, sigma, GO.PER_POINT, shifted=False)
        for a in range(3):
            assert np.isfinite(Ps[a]).all() and np.isfinite(dPs[a]).all()
            assert np.abs(Ps[a].sum(-1) - 1.0).max() <= 1e-14
            d = np.asarray(tr, dtype=np.float64)[:, :, a, None] - np.linspace(-1.0, 1.0, G)
            normal = np.exp(-d * d / (2.0 * sigma * sigma)) > 1e-290
            wmax = np.abs(d / (sigma * sigma)).max(-1, keepdims=True)
            ok = np.isfinite(Pp[a]).all(-1) & np.isfinite(dPp[a]).all(-1)        # [B,N]: the plain row is finite
            rows, nans = rows + int(ok.sum()), nans + int((~ok).sum())
            use = ok[..., None] & normal
            assert use.sum() > 0.2 * use.size
            assert (np.abs(Ps[a] - Pp[a])[use] <= 1e-12 * Pp[a][use]).all()
            assert (np.abs(dPs[a] - dPp[a])[use] <= 1e-12 * (Pp[a] * wmax)[use]).all()
    assert rows > 1000 and nans > 0, "the clouds should hold both kinds of rows"
    for mode in (GO.NONE, GO.ANALYTICAL):                                         # no quotient: nothing is shifted
        for s, p in zip(GO.tables(tr, G, sigma, mode), GO.tables(tr, G, sigma, mode, shifted=False)):
            assert all(np.array_equal(x, y) for x, y in zip(s, p))


def test_oracle_is_finite_where_every_gaussian_of_a_point_underflows():
    import test_gauss_voxels_gpu as TG

    B, N, G, sigma, mode, tr, dvox = TG.case_inputs("u64")
    assert (G, mode) == (64, GO.PER_POINT) and abs(sigma * G - 0.5) < 1e-15
    assert np.array_equal(tr[0, :len(GO.SPECIAL)], GO.SPECIAL.astype(np.float32))
    with np.errstate(invalid="ignore"):
        plain = np.einsum("bnz,bny,bnx->bzyx", *GO.tables(tr, G, sigma, mode, shifted=False)[0], optimize=True)
    assert np.isnan(plain).any(), "the case should be one the plain quotient cannot compute"
    raw = GO.raw_separable(tr, G, sigma, mode)
    dtr = GO.grad_separable(tr, G, sigma, mode, dvox, raw)
    assert np.isfinite(raw).all() and np.isfinite(dtr).all()
    assert abs(raw.sum() - B * N) <= 1e-12 * B * N                                # every point's whole mass is on the grid
    assert (np.abs(dtr[0, list(GO.OUTSIDE)]).max(-1) > 0.1).all()                  # the outside points have a gradient
    # where the literal form is finite it still is the separable one (G = 17: exp's argument stays above -745)
    B, N, G, sigma, mode, tr, _ = TG.case_inputs("u17")
    lit, _ = GO.pointcloud2voxels_literal(tr, G, sigma, mode)
    sep = GO.raw_separable(tr, G, sigma, mode)
    assert np.isfinite(lit).all() and np.abs(lit[..., 0] - sep.transpose(0, 2, 1, 3)).max() <= 1e-13 * sep.max()


def test_fp32_chain_leaves_room_at_the_asserted_workload_shapes_only():
    """How much of the parity bound an honest fp32 sum in index order uses up by itself at the workload's point count.  The
    GPU file asserts raw only where that is at most a third (LARGE) and reports where it is more (REPORTED)."""
    import test_gauss_voxels_gpu as TG

    # a chain of few terms is the fp64 sum to fp32's precision
    B, N, G, sigma, mode, tr, _ = TG.case_inputs("g17")
    assert GO.fraction_of_bound(GO.raw_fp32_chain(tr, G, sigma, mode), GO.raw_separable(tr, G, sigma, mode)) < 0.05
    got = {}
    for tag in TG.ids(TG.LARGE + TG.REPORTED + TG.CHAIN_ONLY + TG.CLIP):
        B, N, G, sigma, mode, tr, _ = TG.case_inputs(tag)
        got[tag] = GO.fraction_of_bound(GO.raw_fp32_chain(tr, G, sigma, mode), GO.raw_separable(tr, G, sigma, mode))
        print("%s: an fp32 chain in index order is at %.3f of the bound" % (tag, got[tag]))
    for tag in TG.ids(TG.LARGE + TG.CLIP):
        assert got[tag] <= 1.0 / 3.0, (tag, got[tag])
    assert 0.05 < got["big32"] < 0.2 and 0.02 < got["big40"] < 0.1                # G = 32, N = 8000 and G = 40, N = 2100, sigma_rel 1
    assert 0.6 < got["big32_wide"] < 0.9 and 0.6 < got["big32_wide_none"] < 0.9   # G = 32, N = 8000, sigma_rel 3


def test_normalise_mode_follows_the_reference_precedence():
    from oracle import dpc_oracle as O

    assert GO.normalise_mode(O.Cfg()) == GO.ANALYTICAL                                    # default_config.yaml:51-52
    assert GO.normalise_mode(O.Cfg(pc_normalise_gauss=True, pc_normalise_gauss_analytical=True)) == GO.PER_POINT
    assert GO.normalise_mode(O.Cfg(pc_normalise_gauss_analytical=False)) == GO.NONE


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_prototypes_and_abi_number():
    from dpc.render import _native as N

    L = N.lib()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert L.dpc_abi_version() == N.ABI_VERSION == 15 and "#define DPC_ABI_VERSION 15" in text
    flat = re.sub(r"\s+", " ", text)
    assert ("int dpc_gauss_voxels_fwd(const DpcParams* p, const float* tr, double sigma, int normalise, float* raw, float* vox, "
            "void* stream);") in flat
    assert ("int dpc_gauss_voxels_bwd(const DpcParams* p, const float* tr, double sigma, int normalise, const float* raw, "
            "const float* dvox, float* dtr, void* stream);") in flat
    for name, value in (("DPC_GAUSS_NORM_NONE", 0), ("DPC_GAUSS_NORM_ANALYTICAL", 1), ("DPC_GAUSS_NORM_PER_POINT", 2),
                        ("DPC_GAUSS_MAX_SIDE", 64)):
        assert "#define %s %d" % (name, value) in text and getattr(N, name) == value
    args = dict((n, a) for n, _, a in N._FUNCTIONS)
    for name, pointers in (("dpc_gauss_voxels_fwd", 4), ("dpc_gauss_voxels_bwd", 5)):
        assert name in N.SYMBOLS and hasattr(L, name)
        assert args[name][2] is ctypes.c_double and args[name][3] is ctypes.c_int
        assert sum(a is ctypes.c_void_p for a in args[name]) == pointers


def _params(B=1, N=4, D=8, H=8, W=8, replicas=1, index=None):
    from dpc.render import _native as N_

    return N_.DpcParams(B, N, D, H, W, 0, 0, 2.0, 1.875, 1e-5, 10.0, replicas, 0, index)


def test_every_refusal_returns_before_a_launch():
    from dpc.render import _native as N

    L = N.lib()
    one = 0x1000   # a non-NULL address that must never be read: every call below returns before a launch
    fwd = lambda P, sigma=0.1, mode=1, tr=one, raw=one, vox=one: L.dpc_gauss_voxels_fwd(
        ctypes.byref(P) if P is not None else None, tr, sigma, mode, raw, vox, None)
    bwd = lambda P, sigma=0.1, mode=1, tr=one, raw=one, dvox=one, dtr=one: L.dpc_gauss_voxels_bwd(
        ctypes.byref(P) if P is not None else None, tr, sigma, mode, raw, dvox, dtr, None)
    for call in (fwd, bwd):
        assert call(None) == N.DPC_ERR_NULL
        assert call(_params(D=8, H=8, W=6)) == N.DPC_ERR_SHAPE
        assert call(_params(D=6, H=8, W=8)) == N.DPC_ERR_SHAPE
        assert call(_params(replicas=2)) == N.DPC_ERR_SHAPE
        assert call(_params(index=one)) == N.DPC_ERR_SHAPE
        for sigma in (0.0, -0.1, float("nan"), float("inf")):
            assert call(_params(), sigma=sigma) == N.DPC_ERR_SHAPE
        for mode in (-1, 3):
            assert call(_params(), mode=mode) == N.DPC_ERR_SHAPE
        assert call(_params(B=-1)) == N.DPC_ERR_SHAPE and call(_params(N=-1)) == N.DPC_ERR_SHAPE
        assert call(_params(D=65, H=65, W=65)) == N.DPC_ERR_LDS
        assert call(_params(B=0)) == 0                       # nothing to do, nothing launched, pointers not looked at
        assert call(_params(B=0), tr=None) == 0
    assert fwd(_params(), vox=None) == N.DPC_ERR_NULL
    assert fwd(_params(), tr=None) == N.DPC_ERR_NULL
    for missing in ("tr", "raw", "dvox", "dtr"):
        assert bwd(_params(), **{missing: None}) == N.DPC_ERR_NULL
    assert bwd(_params(N=0)) == 0                            # an empty gradient: nothing to write


# ------------------------------------------------------------------------------------------------------ Python
def test_python_refusals_come_before_the_device():
    import dpc.render as R
    from oracle import dpc_oracle as O

    pc, q = torch.zeros(1, 4, 3), torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    with pytest.raises(NotImplementedError, match="vox_size_z"):
        R.pointcloud_project_exact(O.Cfg(vox_size=16, vox_size_z=8), pc, q, 0.1)
    with pytest.raises(NotImplementedError, match="vox_size_z"):
        R.pointcloud2voxels(O.Cfg(vox_size=16, vox_size_z=8), pc, 0.1)
    with pytest.raises(NotImplementedError, match="pose_quaternion"):
        R.pointcloud_project_exact(O.Cfg(vox_size=16, pose_quaternion=False), pc, q, 0.1)
    with pytest.raises(NotImplementedError, match="drc_logsum"):
        R.pointcloud_project_exact(O.Cfg(vox_size=16, drc_logsum=False), pc, q, 0.1)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            R.pointcloud2voxels(O.Cfg(vox_size=16), pc, sigma)
    with pytest.raises(RuntimeError, match="MI355X only"):   # no CPU path, no fall-back
        R.pointcloud2voxels(O.Cfg(vox_size=16), pc, 0.1)
    assert R._gauss_normalise(O.Cfg()) == 1
    assert R._gauss_normalise(O.Cfg(pc_normalise_gauss=True)) == 2
    assert R._gauss_normalise(O.Cfg(pc_normalise_gauss_analytical=False)) == 0


def test_exports_and_the_alias():
    import dpc.render as R
    import util.point_cloud_to as overlay

    assert "pointcloud2voxels" in R.__all__ and "pointcloud_project_exact" in R.__all__
    assert overlay.pointcloud2voxels is R.pointcloud2voxels
    assert overlay.pointcloud_project_exact is R.pointcloud_project_exact
    assert R.pointcloud_project is R.pointcloud_project_fast and overlay.pointcloud_project is R.pointcloud_project_fast


def test_train_step_refusals_name_pc_fast():
    from dpc.harness import TrainStep, chair_unsupervised

    small = dict(vox_size=16, pc_num_points=32, pc_fast=False, batch_size=1, step_size=2, input_shape=[32, 32, 3], z_dim=16,
                 fc_dim=16, f_dim=4)
    images, masks = torch.zeros(2, 3, 32, 32), torch.zeros(2, 1, 32, 32)
    step = TrainStep(chair_unsupervised(**small), "cpu", capturable=True, fused_adam=False)
    with pytest.raises(NotImplementedError, match="pc_fast"):
        step.capture(images, masks)
    with pytest.raises(NotImplementedError, match="pc_fast"):
        step.capture_compute(images, masks)
    for key in ("proj_depth_weight", "drc_weight"):
        sup = TrainStep(chair_unsupervised(pose_predict_num_candidates=1, **dict(small, **{key: 1.0})), "cpu", fused_adam=False)
        with pytest.raises(NotImplementedError, match="pc_fast"):
            sup.loss(images, masks, depths=torch.zeros(2, 16, 16, 1))
