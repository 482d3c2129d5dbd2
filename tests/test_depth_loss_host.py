"""The expected-depth loss without a GPU: the fp64 oracle of tests/depth_loss_oracle.py against the reference's own DRC
functions (F20, tests/golden/make_golden_depth_loss.py) and against oracle/dpc_oracle.py's proj_depth, the subsample and
max_dataset_depth rules on a constructed image, the refusals of dpc.render.proj_depth_loss, and the C ABI's bookkeeping."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import depth_loss_oracle as DO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpc_render.h")
NEW_SYMBOLS = ("dpc_depth_workspace_bytes", "dpc_depth_loss_fwd", "dpc_depth_loss_bwd")


def f20():
    return dict(np.load(os.path.join(GOLDEN, "f20_depth_loss.npz")))


@pytest.mark.parametrize("i", [0, 1])
def test_oracle_reproduces_the_reference(i):
    """Depth, loss and the gradient w.r.t. the occupancies of the reference's drc_projection -> flip ->
    drc_depth_projection -> add_proj_depth_loss, to 1e-12 (relative to the largest entry)."""
    g = f20()
    occ = torch.from_numpy(g["occ%d" % i]).requires_grad_(True)
    kw = dict(eps=float(g["eps"]), camera_distance=float(g["camera_distance"]), max_depth=float(g["max_depth"]))
    depth, loss = DO.depth_loss(occ, None, None, torch.from_numpy(g["depths%d" % i]), int(g["factor"]),
                                max_dataset_depth=float(g["max_dataset_depth"]), **kw)
    loss.backward()
    for got, ref, what in ((depth.detach().numpy(), g["depth%d" % i], "depth"), (loss.item(), g["loss%d" % i], "loss"),
                           (occ.grad.numpy(), g["grad%d" % i], "grad")):
        err = np.abs(np.asarray(got) - ref).max()
        assert err <= 1e-12 * max(1.0, np.abs(ref).max()), (what, err)
    sub = DO.subsample(torch.from_numpy(g["depths%d" % i]), int(g["factor"]), float(g["max_depth"]), float(g["max_dataset_depth"]))
    assert np.array_equal(sub.numpy(), g["gt_small%d" % i])
    assert float(g["max_depth"]) != float(g["max_dataset_depth"]) and (g["occ%d" % i] == 0).mean() > 0.4
    assert (g["occ%d" % i] > 1.0 - float(g["eps"])).any()


def test_subsample_and_background_rules():
    """g[y,x] = depths[f*y, f*x] (the top-left pixel of every f x f window), and the dataset's background value becomes
    max_depth only when the two differ."""
    img = torch.arange(16, dtype=torch.float64).reshape(1, 4, 4)
    assert DO.subsample(img, 2).tolist() == [[[0.0, 2.0], [8.0, 10.0]]]
    assert DO.subsample(img, 1).equal(img) and DO.subsample(img, 4).tolist() == [[[0.0]]]
    assert DO.subsample(img, 2, max_depth=7.5, max_dataset_depth=10.0).tolist() == [[[0.0, 2.0], [8.0, 7.5]]]
    assert DO.subsample(img, 2, max_depth=10.0, max_dataset_depth=10.0).tolist() == [[[0.0, 2.0], [8.0, 10.0]]]
    # a pixel the subsample skips is never looked at
    assert DO.subsample(img, 2, max_depth=7.5, max_dataset_depth=5.0).tolist() == [[[0.0, 2.0], [8.0, 10.0]]]
    depth = torch.zeros(1, 2, 2, dtype=torch.float64)
    w = torch.tensor([3.0], dtype=torch.float64)
    assert DO.loss_of_depth(depth, img, 2).item() == 0.5 * (4.0 + 64.0 + 100.0)
    assert DO.loss_of_depth(depth, img, 2, w).item() == 9.0 * 0.5 * (4.0 + 64.0 + 100.0)


def test_oracle_depth_is_the_chain_oracles_proj_depth():
    """The node starts from grid_wh: the chain of oracle/dpc_oracle.py cut after the W and H passes and finished by this
    oracle gives the chain's own proj_depth."""
    from oracle import dpc_oracle as O

    cfg = O.Cfg(vox_size=16, pc_gauss_kernel_size=7)
    pc, q, s, _, _, _ = O.synth_inputs(2, 300, 16, seed=5)
    kern = O.smoothing_kernel(cfg, 1.1)
    ref = O.pointcloud_project_fast(cfg, pc, q, None, None, kern, scaling_factor=s)
    vox = torch.clamp(ref["voxels_raw"].unsqueeze(1), 0.0, 1.0)
    grid_wh = O.smoothen_voxels3d(cfg, vox, kern[:2]).squeeze(1)
    depth = DO.depth_map(grid_wh, s.reshape(-1), kern[2].reshape(-1), cfg.drc_logsum_clip_val, cfg.camera_distance, cfg.max_depth)
    want = ref["proj_depth"][..., 0]
    assert depth.shape == want.shape and float((depth - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(want.min()) < 0.9 * cfg.max_depth   # some rays hit the object


def _outputs(S=2, G=8):
    import dpc.render as R

    return R.ProjectionOutputs(torch.zeros(S, G, G, 1), lambda: {"proj_depth": torch.zeros(S, G, G, 1)})


def test_refusals_name_their_key():
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    cfg = chair_unsupervised(vox_size=8)
    out = _outputs()
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt"):
        R.proj_depth_loss(chair_unsupervised(vox_size=8, pc_gauss_filter_gt=True), out, torch.zeros(2, 8, 8, 1))
    with pytest.raises(ValueError, match="integer multiple"):
        R.proj_depth_loss(cfg, out, torch.zeros(2, 12, 12, 1))
    with pytest.raises(ValueError, match="integer multiple"):
        R.proj_depth_loss(cfg, out, torch.zeros(2, 1, 16, 8))
    with pytest.raises(NotImplementedError, match="pose_predict_num_candidates"):
        R.proj_depth_loss(cfg, _outputs(S=8), torch.zeros(2, 8, 8, 1))
    with pytest.raises(ValueError, match="depths must be"):
        R.proj_depth_loss(cfg, out, torch.zeros(2, 8, 8, 3, 1))
    with pytest.raises(TypeError, match="pointcloud_project_fast"):
        R.proj_depth_loss(cfg, {"proj": out["proj"]}, torch.zeros(2, 8, 8, 1))
    with pytest.raises(TypeError, match="pointcloud_project_fast"):
        R.project_depth({"proj": out["proj"]})


def test_staged_outputs_take_the_torch_route():
    """Outputs that did not come from the fused path (a Gaussian beyond its window): the same numbers from proj_depth."""
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    g = torch.Generator().manual_seed(3)
    pred = 2.0 + torch.rand(2, 4, 4, 1, generator=g, dtype=torch.float64)
    depths = 2.0 + torch.rand(2, 1, 8, 8, generator=g, dtype=torch.float64)
    depths[0, 0, 0, 0] = 10.0
    w = torch.tensor([0.5, 2.0], dtype=torch.float64)
    out = R.ProjectionOutputs(torch.zeros(2, 4, 4, 1), lambda: {"proj_depth": pred})
    for cfg_kw in (dict(), dict(max_depth=7.5, max_dataset_depth=10.0)):
        cfg = chair_unsupervised(vox_size=4, **cfg_kw)
        got = R.proj_depth_loss(cfg, out, depths, w)
        ref = DO.loss_of_depth(pred[..., 0], depths[:, 0], 2, w, cfg.max_depth, cfg.get("max_dataset_depth", cfg.max_depth))
        assert abs(got.item() - ref.item()) <= 1e-13 * ref.item()
    assert R.project_depth(out) is pred


def test_header_and_binding_agree_on_the_new_symbols():
    from dpc.render import _native

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(dpc_depth_\w+)\s*\(([^;]*?)\)\s*;", text)}
    assert sorted(protos) == sorted(NEW_SYMBOLS)
    L = _native.lib()
    assert L.dpc_abi_version() == 15
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


def test_shape_errors_come_before_any_launch():
    """Refusals of the C entry points need no device: they return before anything is enqueued."""
    from dpc.render import _native

    L = _native.lib()
    P = _native.DpcParams(2, 0, 32, 16, 16, 0, 0, 2.0, 1.875, 1e-5, 10.0, 1, 0, None, None, None, None, None)
    ref = ctypes.byref(P)
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    SHAPE = _native.DPC_ERR_SHAPE
    assert L.dpc_depth_loss_fwd(ref, one, None, None, one, 0, 10.0, None, one, one, one, None) == SHAPE      # f < 1
    assert L.dpc_depth_loss_fwd(ref, one, None, None, one, 65, 10.0, None, one, one, one, None) == SHAPE     # f * H > 1024
    assert L.dpc_depth_loss_fwd(ref, one, None, None, one, 1, 10.0, None, one, one, None, None) == SHAPE     # gt without loss
    assert L.dpc_depth_loss_fwd(ref, one, None, None, one, 1, 10.0, None, one, None, one, None) == SHAPE     # ... without tiles
    assert L.dpc_depth_loss_fwd(ref, one, None, None, None, 1, 10.0, None, None, None, None, None) == SHAPE  # nothing asked for
    assert L.dpc_depth_loss_bwd(ref, one, None, None, None, 1, 10.0, None, None, None, one, None, one, None) == SHAPE
    assert L.dpc_depth_loss_bwd(ref, one, None, None, one, 0, 10.0, None, None, None, one, None, one, None) == SHAPE
    assert L.dpc_depth_loss_fwd(ref, None, None, None, None, 1, 10.0, None, one, None, None, None) == _native.DPC_ERR_NULL
    assert L.dpc_depth_loss_bwd(ref, one, None, None, one, 1, 10.0, None, None, None, None, None, one, None) == _native.DPC_ERR_NULL
    assert L.dpc_depth_loss_fwd(None, one, None, None, None, 1, 10.0, None, one, None, None, None) == _native.DPC_ERR_NULL
    # workspace: the ds partials and tickets; a grid more for the depths and kernel lengths the generic backward serves
    small = L.dpc_depth_workspace_bytes(ref)
    assert 0 < small <= 4096
    P24 = _native.DpcParams(2, 0, 24, 16, 16, 0, 0, 2.0, 1.875, 1e-5, 10.0, 1, 0, None, None, None, None, None)
    assert L.dpc_depth_workspace_bytes(ctypes.byref(P24)) >= small + 2 * 24 * 16 * 16 * 4
    P.taps_z = 33
    assert L.dpc_depth_workspace_bytes(ref) >= small + 2 * 32 * 16 * 16 * 4
    assert L.dpc_depth_workspace_bytes(None) == 0
