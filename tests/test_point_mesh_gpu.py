"""The point-to-mesh distance kernel and the F-score on the GPU, against the exact values of the fixture f28_point_mesh.npz.

Tolerance.  A squared distance may differ from the exact value by 8 * max_ratio units of 2^-52 S^2 (S the largest absolute
coordinate of the row): max_ratio is the worst error of the numpy oracle against exact rational arithmetic over the
fixture's cases, recorded by tests/golden/make_golden_point_mesh.py (it is asserted <= 16 there); the factor 8 allows the
kernel another formulation and fused multiply-adds.  It is never derived from the kernel's own output."""
import numpy as np
import pytest
import torch

import dpc.render as R
import point_mesh_oracle as O
from dpc.render import _native

pytestmark = pytest.mark.gpu

BLOCK, TILE = _native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE
SINGLE = ("regions", "regions_p32", "on_triangle", "degenerate_only", "degenerate_nearest", "tile_m1", "tile", "tile_p1", "tile_2p1",
          "cross", "split", "mm", "sliver", "ico", "nan_without")


@pytest.fixture(scope="module")
def f28(golden):
    return golden("f28_point_mesh.npz")


def case(f28, name):
    return f28[name + "_P"], (f28[name + "_V"], f28[name + "_F"]), f28[name + "_d2"]


def close(f28, got, want, P, V):
    """got (a device tensor) within the tolerance of the exact values; +inf where they are."""
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all() and (got[~fin] == np.inf).all()
    err = np.abs(got[fin] - want[fin]) / O.unit(P, V)
    worst = float(err.max()) if fin.any() else 0.0
    print("worst error %.3f units, allowed %.3f" % (worst, 8.0 * float(f28["max_ratio"])))
    assert worst <= 8.0 * float(f28["max_ratio"])
    assert (got >= 0).all()


def status():
    return R.check_status()


@pytest.mark.parametrize("name", SINGLE)
def test_cases_one_row_each(f28, name):
    P, mesh, want = case(f28, name)
    status()
    d2, = R.point_mesh_distance([P], [mesh], squared=True)
    close(f28, d2, want, P, mesh[0])
    assert status() == 0
    d, = R.point_mesh_distance([P], [mesh])
    assert torch.equal(d, torch.sqrt(d2))                                    # bit for bit
    if name == "on_triangle":
        assert (d2[:6] == 0).all() and float(d2[6]) == 0.0625
    if name == "ico":
        Rr, r = f28["ico_radii"]
        assert (d.cpu().numpy() >= r - Rr - np.sqrt(8.0 * float(f28["max_ratio"]) * O.unit(P, mesh[0]))).all()


def test_point_block_boundaries(f28):
    P, mesh, want = case(f28, "blocks")
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1):
        d2, = R.point_mesh_distance([P[:n]], [mesh], squared=True)
        close(f28, d2, want[:n], P, mesh[0])
    alone = [R.point_mesh_distance([P[:n]], [mesh], squared=True)[0] for n in (1, BLOCK - 1, BLOCK, BLOCK + 1)]
    assert all(torch.equal(a, alone[-1][:len(a)]) for a in alone)


def test_non_finite_faces_and_points(f28):
    P, mesh, want = case(f28, "nan_among")
    status()
    d2, = R.point_mesh_distance([P], [mesh], squared=True)
    clean, = R.point_mesh_distance([P], [(f28["nan_without_V"], f28["nan_without_F"])], squared=True)
    assert status() == _native.DPC_STATUS_NONFINITE
    assert torch.equal(d2, clean)
    close(f28, d2, want, P, mesh[0])
    P, mesh, want = case(f28, "nan_only")
    d2, = R.point_mesh_distance([P], [mesh], squared=True)
    assert (d2 == float("inf")).all() and status() == _native.DPC_STATUS_NONFINITE
    good = case(f28, "regions")
    bad = good[0].copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match=r"clouds\[1\] holds a NaN or inf coordinate"):
        R.point_mesh_distance([good[0], bad], [good[1]], mesh_of=[0, 0])
    assert status() == 0


def ragged(f28):
    """Five rows over two meshes, one row without points, fp32 points on fp64 vertices and fp64 points on fp32 vertices;
    the second mesh's vertex and face ranges do not start at 0."""
    tri, soup = case(f28, "regions")[1], case(f28, "tile_p1")[1]
    clouds = [f28["regions_P"], f28["regions_p32_P"], f28["tile_p1_P"], np.zeros((0, 3)), f28["cross_P"]]
    want = [f28["regions_d2"], f28["regions_p32_d2"], f28["tile_p1_d2"], np.zeros(0), f28["cross_d2"]]
    return clouds, [tri, soup], [0, 0, 1, 1, 0], want


def test_a_ragged_batch_in_one_call(f28):
    clouds, meshes, mesh_of, want = ragged(f28)
    assert clouds[1].dtype == np.float32 and meshes[0][0].dtype == np.float64 and meshes[1][0].dtype == np.float32
    got = R.point_mesh_distance(clouds, meshes, mesh_of, squared=True)
    assert [len(g) for g in got] == [len(w) for w in want]
    for g, w, c, k in zip(got, want, clouds, mesh_of):
        close(f28, g, w, c, meshes[k][0])
    # sixty one-triangle meshes, one row each
    T, P = f28["random_T"], f28["random_P"]
    F1 = np.array([[0, 1, 2]])
    got = R.point_mesh_distance(list(P), [(t, F1) for t in T], squared=True)
    for k in range(len(T)):
        close(f28, got[k], f28["random_d2"][k], P[k], T[k])
    assert R.point_mesh_distance([], [], squared=True) == []


def test_order_and_batching_do_not_change_a_bit(f28):
    """The same rows in another order; and a row that takes the split path (3 points, several chunks of faces) issued alone
    and together with rows whose points fill the device, so that it is not split there."""
    clouds, meshes, mesh_of, _ = ragged(f28)
    base = R.point_mesh_distance(clouds, meshes, mesh_of, squared=True)
    perm = [4, 2, 0, 3, 1]
    other = R.point_mesh_distance([clouds[i] for i in perm], meshes[::-1], [1 - mesh_of[i] for i in perm], squared=True)
    for j, i in enumerate(perm):
        assert torch.equal(other[j], base[i])
    P, mesh, want = case(f28, "split")
    alone, = R.point_mesh_distance([P], [mesh], squared=True)
    rng = np.random.default_rng(3)
    filler = (rng.random((8 * 256 * BLOCK, 3)) - 0.5).astype(np.float32)   # point blocks enough for one chunk per row
    tri = case(f28, "regions")[1]
    both = R.point_mesh_distance([filler, P], [tri, mesh], squared=True)
    assert torch.equal(both[1], alone)
    close(f28, alone, want, P, mesh[0])
    assert torch.equal(both[0], R.point_mesh_distance([filler], [tri], squared=True)[0])


def _rule(preds, gts, gt_of, thr, d_pred=None):
    out = np.zeros((len(preds), len(thr), 3))
    for i, k in enumerate(gt_of):
        dp = O.nearest_d(preds[i], gts[k]) if d_pred is None else d_pred[i]
        out[i] = O.fscore_rule(dp, O.nearest_d(gts[k], preds[i]), thr)
    return out


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), (got, want)


def test_fscore_on_clouds_is_the_rule_exactly():
    rng = np.random.default_rng(11)
    gts = [np.round((rng.random((300, 3)) - 0.5) * 64) / 64, (rng.random((257, 3)) - 0.5).astype(np.float32)]
    preds = [gts[0][:200] + np.array([1 / 64, 0, 0]), (rng.random((150, 3)) - 0.5) * 0.9, gts[1][::2].copy(),
             np.zeros((0, 3), dtype=np.float32), (gts[1][:100] + np.float32(0.01)).astype(np.float32)]
    gt_of = [0, 0, 1, 1, 1]
    thr = [1 / 64, 0.01, 0.05, 0.2]                       # 1 / 64 is a distance of preds[0]: d == tau does not count
    got = R.fscore(preds, gts, thr, gt_of)
    want = _rule(preds, gts, gt_of, thr)
    same(got, want)
    assert got.is_cuda and want[0, 0, 0] < 1.0 and want[2, 0, 0] == 1.0
    assert np.isnan(want[3, :, 0]).all() and (want[3, :, 1] == 0).all() and np.isnan(want[3, :, 2]).all()
    far = R.fscore([np.full((3, 3), 0.4)], [np.full((4, 3), -0.4)], [0.1])
    assert far.cpu().tolist() == [[[0.0, 0.0, 0.0]]]
    assert R.fscore([], [], [0.1]).shape == (0, 1, 3)


def test_fscore_against_meshes_is_exact(f28):
    preds, gt, mesh, thr = [f28["fs_pred0"], f28["fs_pred1"]], f28["fs_gt"], (f28["fs_V"], f28["fs_F"]), f28["fs_thresholds"]
    assert float(f28["fs_margin"]) > 8.0 * float(f28["max_ratio"])      # no exact distance that near to a threshold
    d_pred = [np.sqrt(f28["fs_pred0_d2"]), np.sqrt(f28["fs_pred1_d2"])]
    got = R.fscore(preds, [gt], thr, gt_of=[0, 0], gt_meshes=[mesh])
    want = _rule(preds, [gt], [0, 0], thr, d_pred)
    same(got, want)
    on_clouds = R.fscore(preds, [gt], thr, gt_of=[0, 0]).cpu().numpy()
    assert np.array_equal(on_clouds[:, :, 1], want[:, :, 1]) and (want[:, :, 0] >= on_clouds[:, :, 0]).all()
    assert (want[:, :, 0] > on_clouds[:, :, 0]).any()       # the surface is nearer than its samples


def test_fscore_of_split_grouping_rotation_and_num_points(f28):
    rng = np.random.default_rng(13)
    mesh = (f28["fs_V"], f28["fs_F"])
    M, V, N = 5, 2, 80
    d = rng.normal(size=(M, V, N, 3))
    pts = (d / np.linalg.norm(d, axis=3, keepdims=True) * (0.29 + 0.03 * rng.random((M, V, N, 1)))).astype(np.float32)
    nums = [rng.integers(1, N + 1, V) for _ in range(M)]
    nums[2] = None
    gts = [f28["fs_gt"][m::2] for m in range(M)]
    meshes = [mesh] * M
    thr = [0.0071, 0.0133, 0.0291]
    predictions = [(pts[m], nums[m]) for m in range(M)]
    q = np.array([[0.9, 0.1, -0.3, 0.2]])
    for rot in (None, q):
        for gm in (None, meshes):
            all_ = R.fscore_of_split(predictions, gts, thr, reference_rotation=rot, gt_meshes=gm)
            one = R.fscore_of_split(predictions, gts, thr, reference_rotation=rot, gt_meshes=gm, models_per_call=1)
            two = R.fscore_of_split(predictions, gts, thr, reference_rotation=rot, gt_meshes=gm, models_per_call=2)
            assert all_.shape == (M, V, 3, 3) and all_.dtype == np.float64
            assert all_.tobytes() == one.tobytes() == two.tobytes()
            # the same views prepared by hand: truncated, rotated, one fscore call
            views, gt_of = [], []
            for m in range(M):
                p = torch.from_numpy(pts[m])
                if rot is not None:
                    p = R._split._rotate(p, R._split._host_unit_quaternion(rot), torch.device("cuda"))
                for i in range(V):
                    views.append(p[i] if nums[m] is None else p[i, :int(nums[m][i])])
                    gt_of.append(m)
            by_hand = R.fscore(views, gts, thr, gt_of, gm).cpu().numpy().reshape(M, V, 3, 3)
            assert all_.tobytes() == by_hand.tobytes()
            if rot is None and gm is None:
                same(all_.reshape(M * V, 3, 3), _rule([v.numpy() for v in views], gts, gt_of, thr))
    plain = R.fscore_of_split(predictions, gts, thr)
    assert not np.array_equal(plain, R.fscore_of_split(predictions, gts, thr, reference_rotation=q))
    assert not np.array_equal(plain, R.fscore_of_split([(pts[m], None) for m in range(M)], gts, thr))
