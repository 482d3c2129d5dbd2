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

Beyond those nine cases, the tables below walk the paths that they leave out, each named where it is listed: the chunk,
batch, wave and workgroup tails of the four instantiations (TAILS), the grid widths next to a tile edge and the degenerate
ones (WIDTHS), the arguments that underflow in fp32 under pc_normalise_gauss (UNDERFLOW), the workload's point count
(LARGE), a clip that saturates a sizeable share of the grid (CLIP), clouds of a batch against the same clouds alone, and
the Python layer's conversions.
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

# Chunk tails of the forward (128 points a chunk, two per MFMA step, kBatch steps a batch: 2 in fwd<4>, 4 in fwd<1>; what
# is left of a chunk goes through the remainder loop) and wave / workgroup tails of the backward (32 points a wave, 128 a
# workgroup).  fwd<4> and bwd<32> at G = 40:
#   N = 2    1 step: the remainder loop alone             N = 5    3 steps: one batch, then the remainder loop
#   N = 127  an odd chunk, 64 steps, a partly live wave   N = 128  exactly one chunk and one workgroup
#   N = 130  a second chunk of 2 points                   N = 163  a second workgroup whose second wave is partly live
#   N = 257  three chunks, three workgroups
# fwd<1> and bwd<16> at G = 24:
#   N = 3    2 steps and N = 6, 3 steps: the remainder loop alone           N = 127, 128 as above
#   N = 134  a tail chunk of 6 points: 3 leftover steps   N = 163  a tail chunk of 35: four batches, then 2 leftover steps
TAILS = [("t40_n2", 1, 2, 40, 1.0, GO.PER_POINT, 20),
         ("t40_n5", 1, 5, 40, 3.0, GO.NONE, 21),
         ("t40_n127", 1, 127, 40, 0.5, GO.ANALYTICAL, 22),
         ("t40_n128", 1, 128, 40, 1.0, GO.NONE, 23),
         ("t40_n130", 1, 130, 40, 3.0, GO.PER_POINT, 24),
         ("t40_n163", 1, 163, 40, 3.0, GO.ANALYTICAL, 25),
         ("t40_n257", 1, 257, 40, 1.0, GO.ANALYTICAL, 26),
         ("t40_n130_b3", 3, 130, 40, 0.5, GO.NONE, 27),
         ("t24_n3", 1, 3, 24, 3.0, GO.ANALYTICAL, 30),
         ("t24_n6", 1, 6, 24, 1.0, GO.PER_POINT, 31),
         ("t24_n127", 1, 127, 24, 0.5, GO.NONE, 32),
         ("t24_n128", 1, 128, 24, 3.0, GO.PER_POINT, 33),
         ("t24_n134", 1, 134, 24, 1.0, GO.ANALYTICAL, 34),
         ("t24_n163", 1, 163, 24, 1.0, GO.NONE, 35)]

# Widths.  G = 1, 2, 3: a 32-row tile of the backward holds many planes (its row walk wraps many times per tile) and
# centre() has its own branch for G = 1; every voxel is clipped at G = 1 in all modes and at G = 2 under PER_POINT, and
# there the gradient must be exactly zero.  G = 31, 33, 63: one dead, or one live, row and column next to a tile edge;
# G = 33 runs fwd<4> with three z groups, the last holding one live plane.  All clouds are GO.points with its special
# points (N = 20 has room for them).  G = 33 is run under PER_POINT, not NONE: unnormalised, the special point
# (0.5, -0.5, 0.25) sits exactly on a voxel centre of that grid and raw there is 1 to the last bit.
WIDTHS = [("w1_none", 1, 20, 1, 1.0, GO.NONE, 40),
          ("w1_ana", 1, 20, 1, 1.0, GO.ANALYTICAL, 41),
          ("w1_pp", 1, 20, 1, 1.0, GO.PER_POINT, 42),
          ("w2_none", 1, 20, 2, 1.0, GO.NONE, 43),
          ("w2_ana", 1, 20, 2, 1.0, GO.ANALYTICAL, 44),
          ("w2_pp", 1, 20, 2, 1.0, GO.PER_POINT, 45),
          ("w3_none", 1, 20, 3, 1.0, GO.NONE, 46),
          ("w3_ana", 1, 20, 3, 0.5, GO.ANALYTICAL, 47),
          ("w3_pp", 1, 20, 3, 3.0, GO.PER_POINT, 48),
          ("w8", 1, 20, 8, 1.0, GO.NONE, 49),
          ("w16", 1, 20, 16, 1.0, GO.PER_POINT, 50),
          ("w31", 1, 20, 31, 3.0, GO.ANALYTICAL, 51),
          ("w33", 1, 20, 33, 0.5, GO.PER_POINT, 52),
          ("w63", 1, 20, 63, 1.0, GO.NONE, 53)]
ALL_CLIPPED = ("w1_none", "w1_ana", "w1_pp", "w2_pp")

# pc_normalise_gauss with sigma_rel = 0.5: the largest exponent of the point at -1.4 is -92 at G = 17 (a denormal in fp32),
# -184 at G = 24, -512 at G = 40 and -1311 at G = 64 (all zero in fp32, the last zero in fp64 too).  The kernels subtract
# the point's largest exponent before expf; without that these points' tables are 0 / 0.
UNDERFLOW = [("u17", 1, 64, 17, 0.5, GO.PER_POINT, 11),
             ("u24", 1, 64, 24, 0.5, GO.PER_POINT, 11),
             ("u40", 1, 64, 40, 0.5, GO.PER_POINT, 11),
             ("u64", 1, 64, 64, 0.5, GO.PER_POINT, 11)]

# The workload's point count (63 forward chunks a cloud) and 17 chunks / 17 workgroups of the wide instantiations.  An
# honest fp32 chain in index order (GO.raw_fp32_chain) sits at 0.13 and 0.04 of the bound for raw at these two shapes
# (tests/test_gauss_voxels_host.py asserts at most a third), so a failure here means the kernel is wrong.  REPORTED is
# printed, not asserted: the same chain is at 0.72 of the bound there, so the rule cannot judge a kernel at that shape.
LARGE = [("big32", 1, 8000, 32, 1.0, GO.ANALYTICAL, 70),
         ("big40", 1, 2100, 40, 1.0, GO.ANALYTICAL, 71)]
REPORTED = [("big32_wide", 1, 8000, 32, 3.0, GO.ANALYTICAL, 72)]
CHAIN_ONLY = [("big32_wide_none", 1, 8000, 32, 3.0, GO.NONE, 73)]     # host side only, like REPORTED

# A clip that saturates: 15 % of the voxels above 1 at G = 32 (bwd<16>), 10 % at G = 40 (bwd<32>).
CLIP = [("clip32", 1, 1000, 32, 3.0, GO.NONE, 60),
        ("clip40", 1, 2100, 40, 2.0, GO.NONE, 61)]

EVERY = {c[0]: c for c in CASES + TAILS + WIDTHS + UNDERFLOW + LARGE + REPORTED + CHAIN_ONLY + CLIP}
ids = lambda table: [c[0] for c in table]


def case_inputs(tag):
    """(B, N, G, sigma, mode, tr, dvox) of a case, from its seed."""
    _, B, N, G, sigma_rel, mode, seed = EVERY[tag]
    rng = np.random.default_rng(seed)
    tr = GO.points(rng, B, N)
    dvox = rng.standard_normal((B, G, G, G)).astype(np.float32)
    return B, N, G, sigma_rel / G, mode, tr, dvox


@functools.lru_cache(maxsize=None)
def case_data(tag):
    """Inputs and the oracle's answers of a case, computed once and shared (read only)."""
    B, N, G, sigma, mode, tr, dvox = case_inputs(tag)
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


GUARD = 64     # floats of NaN behind every output of c_abi, which the kernels must leave alone


def _guarded(shape):
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), np.nan, device="cuda")
    return flat, flat[:n].view(shape)


def c_abi(c, tr, dvox):
    """(raw, vox, dtr) straight from the two entry points.  Nothing is written behind an output's last element (where a
    backward lane that takes point N for a live one would write its row)."""
    from dpc.render import _native as N

    P = N.DpcParams(c["B"], c["N"], c["G"], c["G"], c["G"], 0, 0, 2.0, 1.875, 1e-5, 10.0, 1)
    shape = (c["B"], c["G"], c["G"], c["G"])
    (raw_all, raw), (vox_all, vox), (dtr_all, dtr) = _guarded(shape), _guarded(shape), _guarded((c["B"], c["N"], 3))
    st = N.stream_ptr(tr.device)
    N.check(N.lib().dpc_gauss_voxels_fwd(ctypes.byref(P), N.ptr(tr), c["sigma"], c["mode"], N.ptr(raw), N.ptr(vox), st), "fwd")
    N.check(N.lib().dpc_gauss_voxels_bwd(ctypes.byref(P), N.ptr(tr), c["sigma"], c["mode"], N.ptr(raw), N.ptr(dvox), N.ptr(dtr), st),
            "bwd")
    torch.cuda.synchronize()
    for name, buf in (("raw", raw_all), ("vox", vox_all), ("dtr", dtr_all)):
        assert bool(torch.isnan(buf[-GUARD:]).all()), "the kernels wrote behind the end of " + name
    return raw, vox, dtr


def mode_cfg(G, mode, **kw):
    from oracle import dpc_oracle as O

    return O.Cfg(vox_size=G, pc_normalise_gauss=mode == GO.PER_POINT, pc_normalise_gauss_analytical=mode == GO.ANALYTICAL, **kw)


def on_device(c):
    return torch.from_numpy(c["tr"]).cuda(), torch.from_numpy(c["dvox"]).cuda()


def check_case(tag):
    """Both entry points against the oracle, the pass-through set, and a second run bit for bit: (raw, vox, dtr)."""
    c = case_data(tag)
    tr, dvox = on_device(c)
    raw, vox, dtr = c_abi(c, tr, dvox)
    close(raw, c["raw"], tag + " raw")
    close(vox, c["vox"], tag + " vox")
    close(dtr, c["dtr"], tag + " dtr")
    mask_dev = ((raw >= 0) & (raw <= 1)).cpu().numpy()
    assert np.array_equal(mask_dev, (c["raw"] >= 0) & (c["raw"] <= 1)), "the pass-through set differs from the oracle's"
    raw2, vox2, dtr2 = c_abi(c, tr, dvox)
    assert torch.equal(raw, raw2) and torch.equal(vox, vox2), "two runs of the forward differ"
    assert torch.equal(dtr, dtr2), "two runs of the backward differ"
    return raw, vox, dtr


@pytest.mark.parametrize("tag", IDS)
def test_entry_points_match_the_oracle_and_repeat_bit_for_bit(tag):
    check_case(tag)


@pytest.mark.parametrize("tag", ids(TAILS))
def test_chunk_wave_and_workgroup_tails(tag):
    check_case(tag)


@pytest.mark.parametrize("tag", ids(WIDTHS))
def test_width_edges(tag):
    c = case_data(tag)
    clipped = c["raw"] > 1.0
    assert clipped.all() == (tag in ALL_CLIPPED), "the case table names the all-clipped cases wrongly"
    raw, vox, dtr = check_case(tag)
    if tag in ALL_CLIPPED:
        assert float(vox.min()) == 1.0 and float(vox.max()) == 1.0
        assert int(torch.count_nonzero(dtr)) == 0, "every voxel is clipped: the gradient is exactly zero"
    else:
        assert float(np.abs(c["dtr"]).max()) > 0.1, "the case has no gradient to compare"


@pytest.mark.parametrize("tag", ids(UNDERFLOW))
def test_underflowing_arguments_under_per_point_normalisation(tag):
    c = case_data(tag)
    G, sigma = c["G"], c["sigma"]
    # the case is in the regime it is named for: the point at -1.4 has no fp32 Gaussian left on its second axis
    top = -((-1.4 + 1.0) ** 2) / (2.0 * sigma * sigma)
    assert np.array_equal(c["tr"][0, GO.OUTSIDE[1]], GO.SPECIAL[GO.OUTSIDE[1]].astype(np.float32)) and top < -87.0
    assert np.isfinite(c["raw"]).all() and np.isfinite(c["dtr"]).all()
    raw, vox, dtr = check_case(tag)
    assert torch.isfinite(raw).all() and torch.isfinite(vox).all() and torch.isfinite(dtr).all()
    # the outside points' own rows are part of what close() compared: finite on both sides, not zero in the oracle, and the
    # points' whole mass is on the grid (under this normalisation the grid sums to the number of points)
    rows = list(GO.OUTSIDE)
    assert (np.abs(c["dtr"][0, rows]).max(axis=1) > 0.1).all(), "an outside point has no gradient to compare"
    assert torch.isfinite(dtr[0, rows]).all()
    assert abs(float(raw.double().sum()) - c["N"]) <= 1e-4 * c["N"]     # fp32 tables, summed here in fp64: a few 1e-7 relative


@pytest.mark.parametrize("tag", ids(LARGE))
def test_workload_sized_clouds(tag):
    check_case(tag)


@pytest.mark.parametrize("tag", ids(REPORTED))
def test_wide_sigma_at_the_workload_size_is_reported_not_judged(tag):
    """An honest fp32 chain alone is at 0.72 of the bound for raw here (tests/test_gauss_voxels_host.py), so the rule cannot
    judge a kernel at this shape: the figures are printed for profiles/gauss_voxels_parity.json, nothing but finiteness is
    asserted."""
    c = case_data(tag)
    tr, dvox = on_device(c)
    for name, dev in zip(("raw", "vox", "dtr"), c_abi(c, tr, dvox)):
        assert torch.isfinite(dev).all()
        print("%s %s: %.2f of the bound (reported, not asserted)" % (tag, name, GO.fraction_of_bound(dev.cpu().numpy(), c[name], TOL)))


@pytest.mark.parametrize("tag", ids(CLIP))
def test_saturated_clip(tag):
    c = case_data(tag)
    clipped = c["raw"] > 1.0
    assert 0.08 < clipped.mean() < 0.5, "the case should clip a sizeable share of the grid, not all of it"
    raw, vox, dtr = check_case(tag)
    on = torch.from_numpy(clipped).cuda()
    assert bool((vox[on] == 1.0).all()), "a clipped voxel is exactly 1"
    assert float(np.abs(c["dtr"]).max()) > 1.0
    # a gradient that arrives at clipped voxels only contributes exactly nothing
    tr, dvox = on_device(c)
    _, _, dead = c_abi(c, tr, torch.where(on, dvox, torch.zeros_like(dvox)))
    assert int(torch.count_nonzero(dead)) == 0 and not bool(torch.isnan(dead).any())


@pytest.mark.parametrize("tag", ["g32_b3", "t40_n130_b3"])      # fwd<1> and bwd<16>, fwd<4> and bwd<32>
def test_a_cloud_of_a_batch_equals_the_cloud_alone_bit_for_bit(tag):
    c = case_data(tag)
    tr, dvox = on_device(c)
    raw, vox, dtr = c_abi(c, tr, dvox)
    assert c["B"] == 3
    for b in range(c["B"]):
        raw1, vox1, dtr1 = c_abi(dict(c, B=1), tr[b:b + 1].contiguous(), dvox[b:b + 1].contiguous())
        assert torch.equal(raw1[0], raw[b]) and torch.equal(vox1[0], vox[b]), "cloud %d alone gives another grid" % b
        assert torch.equal(dtr1[0], dtr[b]), "cloud %d alone gives another gradient" % b


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


def _render_and_grad(cfg, tr, sigma, dvox):
    import dpc.render as R

    out = R.pointcloud2voxels(cfg, tr, sigma)
    (out[..., 0].transpose(1, 2) * dvox).sum().backward()
    return out.detach()


@pytest.mark.parametrize("tag", ["g17", "g40"])
def test_python_layer_converts_dtypes_and_strides(tag):
    """fp64, fp16 and non-contiguous points give the bits of the contiguous fp32 call on the same rounded points, and the
    gradient comes back in the input's dtype and shape."""
    c = case_data(tag)
    cfg, sigma = mode_cfg(c["G"], c["mode"]), c["sigma"]
    tr, dvox = on_device(c)

    def plain(points32):
        leaf = points32.clone().contiguous().requires_grad_(True)
        return _render_and_grad(cfg, leaf, sigma, dvox), leaf.grad

    t64 = (tr.double() * (1.0 + 1e-9)).requires_grad_(True)          # not representable in fp32: the layer rounds
    assert not torch.equal(t64.detach().float().double(), t64.detach())
    out, (ref, gref) = _render_and_grad(cfg, t64, sigma, dvox), plain(t64.detach().float())
    assert out.dtype is torch.float32 and torch.equal(out, ref)
    assert t64.grad.dtype is torch.float64 and t64.grad.shape == t64.shape and torch.equal(t64.grad, gref.double())

    t16 = tr.half().requires_grad_(True)
    out, (ref, gref) = _render_and_grad(cfg, t16, sigma, dvox), plain(t16.detach().float())
    assert torch.equal(out, ref)
    assert t16.grad.dtype is torch.float16 and t16.grad.shape == t16.shape and torch.equal(t16.grad, gref.half())
    assert torch.isfinite(t16.grad).all() and float(t16.grad.abs().max()) > 0

    wide = torch.cat([tr, torch.full_like(tr[..., :1], 7.0)], dim=-1).requires_grad_(True)     # [B,N,4]
    cut = wide[..., :3]
    cut.retain_grad()
    assert not cut.is_contiguous()
    out, (ref, gref) = _render_and_grad(cfg, cut, sigma, dvox), plain(tr)
    assert torch.equal(out, ref)
    assert cut.grad.shape == cut.shape and torch.equal(cut.grad, gref)
    assert wide.grad.shape == wide.shape and torch.equal(wide.grad[..., :3], gref) and float(wide.grad[..., 3].abs().max()) == 0.0
    close(ref, GO.pointcloud2voxels_literal(c["tr"], c["G"], sigma, c["mode"])[1], tag + " voxels of the contiguous fp32 call")


def test_no_grad_does_not_allocate_the_sums_before_the_clip():
    import dpc.render as R

    B, N, G = 2, 64, 64
    cfg = mode_cfg(G, GO.ANALYTICAL)
    tr = torch.from_numpy(GO.points(np.random.default_rng(80), B, N)).cuda().requires_grad_(True)
    grid = B * G * G * G * 4

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - before

    with torch.no_grad():
        out, used = peak(lambda: R.pointcloud2voxels(cfg, tr, 3.0 / G))
    assert out.grad_fn is None and not out.requires_grad
    assert grid <= used < 2 * grid, "no_grad: one grid is allocated, not two (%d bytes for a grid of %d)" % (used, grid)
    again, used = peak(lambda: R.pointcloud2voxels(cfg, tr, 3.0 / G))
    assert used >= 2 * grid, "with a gradient wanted the sums before the clip are kept: the measurement can tell"
    assert torch.equal(again.detach(), out)


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
