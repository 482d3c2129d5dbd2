"""The colour projection and its loss without a GPU: the fp64 oracle of tests/rgb_oracle.py against the reference's own
functions and numpy restatements of its TF-1 lines (F21, tests/golden/make_golden_rgb_loss.py), the integral's two limits
against oracle/dpc_oracle.py's probabilities, the integer-factor sampling rule, the refusals of dpc.render.proj_rgb_loss,
the C ABI's bookkeeping, and the decoder's colour head."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rgb_oracle as RO
from oracle import dpc_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpc_render.h")
NEW_SYMBOLS = ("dpc_rgb_splat_fwd", "dpc_rgb_splat_bwd", "dpc_rgb_loss_fwd", "dpc_rgb_loss_bwd")


def f21():
    return dict(np.load(os.path.join(GOLDEN, "f21_rgb_loss.npz")))


def f21_case(g, i):
    cfg = O.Cfg(vox_size=int(g["vox_size%d" % i]), vox_size_z=int(g["vox_size_z%d" % i]),
                pc_rgb_divide_by_occupancies=bool(g["divide%d" % i]), pc_rgb_clip_after_conv=bool(g["clip_after%d" % i]),
                pc_rgb_divide_by_occupancies_epsilon=float(g["div_eps%d" % i]), drc_logsum_clip_val=float(g["eps%d" % i]))
    kxy, kz = torch.from_numpy(g["kxy%d" % i]), torch.from_numpy(g["kz%d" % i])
    kernel = [kxy.reshape(1, 1, 1, 1, -1), kxy.reshape(1, 1, 1, -1, 1), kz.reshape(1, 1, -1, 1, 1)]
    return cfg, kernel


@pytest.mark.parametrize("i", [0, 1])
def test_oracle_reproduces_the_reference(i):
    """Raw colour grid, colour grid, image and loss of the reference's splat / smoothing / DRC functions and the numpy
    restatement of its TF-1 colour lines, to 1e-12 (relative to the largest entry)."""
    g = f21()
    cfg, kernel = f21_case(g, i)
    tr, rgb, vox = (torch.from_numpy(g[k % i]) for k in ("tr%d", "rgb%d", "vox%d"))
    images, f = torch.from_numpy(g["images%d" % i]), int(g["factor%d" % i])
    parts = {}
    proj, vrgb, loss = RO.rgb_loss(cfg, tr, rgb, vox, kernel, images, f, parts=parts)
    raw = parts["raw"].permute(0, 2, 3, 4, 1)
    for got, ref, what in ((raw.numpy(), g["raw%d" % i], "raw"), (vrgb.numpy(), g["voxels_rgb%d" % i], "voxels_rgb"),
                           (proj.numpy(), g["proj_rgb%d" % i], "proj_rgb"), (loss.item(), g["loss%d" % i], "loss")):
        err = np.abs(np.asarray(got) - ref).max()
        assert err <= 1e-12 * max(1.0, np.abs(ref).max()), (what, err)
    assert np.array_equal(RO.subsample(images, f).numpy(), g["gt_small%d" % i])
    # the fixture reaches what it is meant to: colours above 1 before the clip, points outside the cube, both options
    assert g["raw%d" % i].max() > 1.0 and (np.abs(g["tr%d" % i]) > 0.5).any()
    assert bool(g["divide0"]) and not bool(g["clip_after0"]) and bool(g["clip_after1"]) and int(g["factor0"]) == 2


def test_integral_limits_against_the_chain_oracle():
    """A colour grid of ones integrates to sum_k p_k over all D+1 events of the chain oracle's probabilities, a grid of
    zeros to p_D alone (the white background); rows flipped like the chain's."""
    cfg = O.Cfg(vox_size=12, pc_gauss_kernel_size=5)
    pc, q, s, _, _, _ = O.synth_inputs(2, 200, 12, seed=3)
    ref = O.pointcloud_project_fast(cfg, pc, q, None, None, O.smoothing_kernel(cfg, 0.9), scaling_factor=s)
    vox, probs = ref["voxels"][..., 0], ref["drc_probs"][..., 0]      # probs [D+1,B,H,W], already flipped
    ones = RO.integrate(cfg, torch.ones(2, 3, 12, 12, 12, dtype=torch.float64), vox)
    zeros = RO.integrate(cfg, torch.zeros(2, 3, 12, 12, 12, dtype=torch.float64), vox)
    for c in range(3):
        assert float((ones[..., c] - probs.sum(0)).abs().max()) <= 1e-13
        assert float((zeros[..., c] - probs[-1]).abs().max()) <= 1e-13
    assert float(probs[-1].min()) < 0.9   # some rays hit the object


def test_integer_factor_sampling_rule():
    """g[y,x] = images[f*y, f*x]: the top-left pixel of every f x f window, per channel."""
    img = torch.arange(48, dtype=torch.float64).reshape(1, 4, 4, 3)
    assert RO.subsample(img, 2)[0, :, :, 0].tolist() == [[0.0, 6.0], [24.0, 30.0]]
    assert RO.subsample(img, 2)[0, 1, 1].tolist() == [30.0, 31.0, 32.0]
    assert RO.subsample(img, 1).equal(img) and RO.subsample(img, 4)[0, 0, 0].tolist() == [0.0, 1.0, 2.0]
    proj = torch.zeros(1, 2, 2, 3, dtype=torch.float64)
    want = 0.5 * sum(float(v) ** 2 for y in (0, 2) for x in (0, 2) for v in img[0, y, x])
    assert RO.loss_of_rgb(proj, img, 2).item() == want
    assert RO.loss_of_rgb(proj, img, 2, torch.tensor([3.0], dtype=torch.float64)).item() == 9.0 * want


def _outputs(S=2, G=8):
    import dpc.render as R

    return R.ProjectionOutputs(torch.zeros(S, G, G, 1), lambda: {"tr_pc": torch.zeros(S, 5, 3), "voxels": torch.zeros(S, G, G, G, 1)})


def test_refusals_name_their_key():
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    cfg = chair_unsupervised(vox_size=8)
    out, rgb = _outputs(), torch.zeros(2, 5, 3)
    with pytest.raises(NotImplementedError, match="pc_gauss_filter_gt_rgb"):
        R.proj_rgb_loss(chair_unsupervised(vox_size=8, pc_gauss_filter_gt_rgb=True), out, rgb, torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match="integer multiple"):
        R.proj_rgb_loss(cfg, out, rgb, torch.zeros(2, 12, 12, 3))
    with pytest.raises(ValueError, match="integer multiple"):
        R.proj_rgb_loss(cfg, out, rgb, torch.zeros(2, 3, 16, 8))
    with pytest.raises(NotImplementedError, match="pose_predict_num_candidates"):
        R.proj_rgb_loss(cfg, _outputs(S=8), torch.zeros(8, 5, 3), torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match="images must be"):
        R.proj_rgb_loss(cfg, out, rgb, torch.zeros(2, 8, 8, 1))
    with pytest.raises(TypeError, match="pointcloud_project_fast"):
        R.proj_rgb_loss(cfg, {"proj": out["proj"]}, rgb, torch.zeros(2, 8, 8, 3))
    with pytest.raises(TypeError, match="pointcloud_project_fast"):
        R.project_rgb(cfg, {"proj": out["proj"]}, rgb)
    with pytest.raises(ValueError, match="all_rgb must hold"):
        R.proj_rgb_loss(cfg, out, torch.zeros(2, 4, 3), torch.zeros(2, 8, 8, 3))
    # the projection itself keeps refusing colours, and says where they went
    with pytest.raises(NotImplementedError, match="all_rgb.*project_rgb"):
        R.pointcloud_project_fast(cfg, torch.zeros(2, 5, 3), torch.zeros(2, 4), None, rgb)
    assert out["voxels_rgb"] is None and out["proj_rgb"] is None
    assert {"project_rgb", "proj_rgb_loss", "replicate_rgb"} <= set(R.__all__)


def test_replicate_rgb():
    import dpc.render as R

    rgb = torch.arange(2 * 4 * 3, dtype=torch.float32).reshape(2, 4, 3)
    rep = R.replicate_rgb(rgb, 6)
    assert rep.shape == (6, 4, 3) and all(rep[b].equal(rgb[b // 3]) for b in range(6))     # tf_repeat_0 order
    idx = torch.tensor([[3, 0], [1, 1], [2, 3], [0, 1], [3, 3], [2, 0]], dtype=torch.int32)
    sub = R.replicate_rgb(rgb, 6, idx)
    assert sub.shape == (6, 2, 3) and all(sub[b, j].equal(rgb[b // 3, int(idx[b, j])]) for b in range(6) for j in range(2))
    assert R.replicate_rgb(rgb, 2) is rgb
    with pytest.raises(ValueError, match="multiple"):
        R.replicate_rgb(rgb, 5)


def test_header_and_binding_agree_on_the_new_symbols():
    from dpc.render import _native

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(dpc_rgb_\w+)\s*\(([^;]*?)\)\s*;", text)}
    assert sorted(protos) == sorted(NEW_SYMBOLS)
    L = _native.lib()
    assert L.dpc_abi_version() == 15
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    for name in NEW_SYMBOLS:
        assert name in _native.SYMBOLS
        ret, args = protos[name]
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and ret == "int"
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
    P = _native.DpcParams(2, 10, 32, 16, 16, 0, 0, 2.0, 1.875, 1e-5, 10.0, 1, 0, None, None, None, None, None)
    ref = ctypes.byref(P)
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    SHAPE, NULL = _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL
    fwd, bwd = L.dpc_rgb_loss_fwd, L.dpc_rgb_loss_bwd
    assert fwd(ref, one, one, None, 0.01, 0, one, 0, 0, None, one, one, one, None) == SHAPE      # f < 1
    assert fwd(ref, one, one, None, 0.01, 0, one, 65, 0, None, one, one, one, None) == SHAPE     # f * H > 1024
    assert fwd(ref, one, one, None, 0.01, 0, one, 1, 0, None, one, one, None, None) == SHAPE     # gt without loss
    assert fwd(ref, one, one, None, 0.01, 0, one, 1, 1, None, one, None, one, None) == SHAPE     # ... without tiles
    assert fwd(ref, one, one, None, 0.01, 0, None, 1, 0, None, None, None, None, None) == SHAPE  # nothing asked for
    assert bwd(ref, one, one, None, 0.01, 0, None, 1, 0, None, one, None, None, one, one, None) == SHAPE   # no gradient arrives
    assert bwd(ref, one, one, None, 0.01, 0, one, 0, 0, None, one, None, None, one, one, None) == SHAPE    # f < 1
    assert fwd(ref, None, one, None, 0.01, 0, None, 1, 0, None, one, None, None, None) == NULL
    assert fwd(ref, one, None, None, 0.01, 0, None, 1, 0, None, one, None, None, None) == NULL
    assert bwd(ref, one, one, None, 0.01, 0, one, 1, 0, None, one, None, None, None, one, None) == NULL    # no dvox
    assert bwd(ref, one, one, None, 0.01, 0, one, 1, 0, None, None, None, None, one, one, None) == NULL    # gt without the saved image
    assert fwd(None, one, one, None, 0.01, 0, None, 1, 0, None, one, None, None, None) == NULL
    assert L.dpc_rgb_splat_fwd(ref, None, one, one, None) == NULL and L.dpc_rgb_splat_fwd(ref, one, one, None, None) == NULL
    assert L.dpc_rgb_splat_bwd(ref, one, one, one, None, None, None) == NULL
    assert L.dpc_rgb_splat_fwd(None, one, one, one, None) == NULL
    # the colour node is stage-level: one row of points and colours per cloud
    P.point_replicas = 2
    assert L.dpc_rgb_splat_fwd(ref, one, one, one, None) == SHAPE and L.dpc_rgb_splat_bwd(ref, one, one, one, one, None, None) == SHAPE
    P.point_replicas, P.D = 1, 2000
    assert L.dpc_rgb_splat_fwd(ref, one, one, one, None) == SHAPE
    assert fwd(ref, one, one, None, 0.01, 0, None, 1, 0, None, one, None, None, None) == SHAPE


def test_decoder_returns_colours_under_pc_rgb():
    """Decoder.forward: (points, sigmoid colours [B,N,3]) under pc_rgb -- from the code, or from rgb_deep_decoder of the
    conv features under pc_rgb_deep_decoder (pc_decoder_to.py:44-55); the points alone, as before, under the default."""
    from dpc.harness.config import chair_unsupervised
    from dpc.harness.nets import Decoder

    kw = dict(fc_dim=16, pc_num_points=7)
    code, feat = torch.randn(3, 16, generator=torch.Generator().manual_seed(1)), torch.randn(3, 16, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(0)
    plain = Decoder(chair_unsupervised(**kw))
    torch.manual_seed(0)
    coloured = Decoder(chair_unsupervised(pc_rgb=True, **kw))
    torch.manual_seed(0)
    deep = Decoder(chair_unsupervised(pc_rgb=True, pc_rgb_deep_decoder=True, **kw))
    xyz = plain(code)
    assert isinstance(xyz, torch.Tensor) and xyz.shape == (3, 7, 3)
    assert xyz.equal(torch.tanh(plain.pts_raw_fc(code).reshape(-1, 7, 3)) / 2.0)
    xyz2, rgb = coloured(code)
    assert xyz2.equal(xyz) and rgb.shape == (3, 7, 3) and float(rgb.detach().min()) > 0.0 and float(rgb.detach().max()) < 1.0
    assert rgb.equal(torch.sigmoid(coloured.rgb_raw_dec(code).reshape(-1, 7, 3)))
    xyz3, rgb_deep = deep(code, feat)
    assert xyz3.equal(xyz) and rgb_deep.equal(torch.sigmoid(deep.rgb_raw_dec(deep.rgb_deep_decoder(feat)).reshape(-1, 7, 3)))
    assert not rgb_deep.equal(rgb)
    with pytest.raises(ValueError, match="pc_rgb_deep_decoder"):
        deep(code, torch.zeros(3, 20))
