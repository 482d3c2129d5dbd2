"""CPU side of the unsupervised alignment (no GPU): the host helpers of dpc.render.alignment against the F15 fixture, which
the reference's own code produced (tests/golden/make_golden_alignment.py), the ICP oracle the GPU tests use, and the
argument checks of the ICP's C ABI, which return before anything touches a device.

icp_oracle is a numpy / torch-CPU fp64 restatement of the semantics in include/dpc_render.h (open3d 0.9's point-to-point
registration_icp): brute-force nearest in chunks with d2 = (d0*d0 + d1*d1) + d2*d2, first index on ties, inliers d2 < tau^2,
Umeyama by SVD, points moved in place per update with the same per-row sums as the kernels."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def f15(golden):
    return golden("f15_alignment.npz")


def _apply(U, pts):
    """x' = ((R00 x + R01 y) + R02 z) + t0 per row: the kernels' order, no FMA (numpy evaluates each product apart)."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((U[r, 0] * x + U[r, 1] * y) + U[r, 2] * z) + U[r, 3] for r in range(3)], axis=1)


def _nearest(cur, tgt, chunk=512):
    """(index, d2) of the nearest target of every point, brute force, first minimum."""
    t = torch.from_numpy(tgt)
    idx = np.empty(len(cur), dtype=np.int64)
    d2 = np.empty(len(cur))
    for a in range(0, len(cur), chunk):
        s = torch.from_numpy(cur[a:a + chunk])
        d = t[None, :, :] - s[:, None, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best, j = torch.min(dd, dim=1)   # first minimum, like torch.argmin
        idx[a:a + chunk], d2[a:a + chunk] = j.numpy(), best.numpy()
    return idx, d2


def _umeyama(p, q):
    mp, mq = p.mean(0), q.mean(0)
    sigma = (q - mq).T @ (p - mp) / len(p)
    U, _, Vt = np.linalg.svd(sigma)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    return T


def icp_oracle(src, tgt, max_dist, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """Returns (transform [4,4], fitness, inlier_rmse, iterations)."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    tau2 = max_dist * max_dist
    cur = _apply(T, src)

    def evaluate(cur):
        if len(cur) == 0:
            return 0.0, 0.0, None, None
        idx, d2 = _nearest(cur, tgt)
        inl = d2 < tau2
        n = int(inl.sum())
        if n == 0:
            return 0.0, 0.0, None, None
        return n / len(cur), float(np.sqrt(d2[inl].sum() / n)), cur[inl], tgt[idx[inl]]

    fit, rmse, p, q = evaluate(cur)
    it = 0
    for it in range(1, max_iteration + 1):
        upd = np.eye(4) if p is None else _umeyama(p, q)
        T = upd @ T
        cur = _apply(upd, cur)
        fit0, rmse0 = fit, rmse
        fit, rmse, p, q = evaluate(cur)
        if abs(fit0 - fit) < relative_fitness and abs(rmse0 - rmse) < relative_rmse:
            break
    return T, fit, rmse, (it if max_iteration > 0 else 0)


def rotation(axis, angle):
    from dpc.render.alignment import as_rotation_matrix

    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return as_rotation_matrix(np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])[None])[0]


def shape_cloud(n, rng):
    """An asymmetric test object: a slab, a rod off its corner and a ball, ~1 unit across (ICP has one clear optimum)."""
    k = rng.multinomial(n, [0.5, 0.3, 0.2])
    slab = rng.uniform([-0.5, -0.3, -0.05], [0.5, 0.3, 0.05], size=(k[0], 3))
    rod = rng.uniform([0.3, 0.2, 0.0], [0.4, 0.3, 0.6], size=(k[1], 3))
    ball = rng.normal(size=(k[2], 3)) * 0.08 + [-0.35, -0.1, 0.25]
    return np.concatenate([slab, rod, ball])


# ---------------------------------------------------------------------------------------------------- F15 host helpers
def test_quaternion_from_campos_matches_reference(f15):
    from dpc.render import quaternion_from_campos

    got = np.stack([quaternion_from_campos(c) for c in f15["campos"]])
    assert np.abs(got - f15["campos_quat"]).max() <= 1e-12


def test_rotation_matrix_conversions_match_reference(f15):
    from dpc.render import as_rotation_matrix, from_rotation_matrix

    R = as_rotation_matrix(f15["quats"])
    assert np.abs(R - f15["rotmats"]).max() <= 1e-12
    q = from_rotation_matrix(f15["rotmats"])
    ref = f15["rotmats_quat"]
    nan = np.isnan(ref)
    assert nan.any(), "the fixture must hold the near-180-degree NaN rows"
    assert np.array_equal(np.isnan(q), nan)
    fin = np.isfinite(ref)   # w == 0 exactly gives +-inf in the other three, there as here
    assert np.array_equal(q[~fin & ~nan], ref[~fin & ~nan])
    assert np.abs(q[fin] - ref[fin]).max() <= 1e-12


def test_reference_rotation_matches_compute_alignment(f15):
    from dpc.render import reference_rotation

    got = reference_rotation(f15["cand_rotations"], f15["cand_rmse"])
    assert np.abs(got - f15["reference_rotation"].reshape(4)).max() <= 1e-12


def test_reference_rotation_drops_nan_rows(f15):
    from dpc.render import quat_w_avg_markley, reference_rotation

    rot = f15["cand_rotations"].copy()
    rmse = f15["cand_rmse"]
    best = np.argsort(rmse[np.argmin(rmse.min(1))])[0]
    rot[np.argmin(rmse.min(1)), best] = np.nan   # a NaN row among the selected ones, as from_rotation_matrix makes near 180
    got = reference_rotation(rot, rmse)
    assert np.isfinite(got).all() and abs(np.linalg.norm(got) - 1) < 1e-12
    assert np.abs(quat_w_avg_markley(np.array([[1.0, 0, 0, 0]] * 3)) - [1, 0, 0, 0]).max() < 1e-15


def test_pose_errors_match_run_eval(f15):
    from dpc.render import pose_errors

    err, acc, med = pose_errors(f15["pose_pred"].reshape(-1, 4), f15["pose_cam_pos"].reshape(-1, 3), f15["reference_rotation"])
    assert np.abs(err - f15["pose_angle_error"].reshape(-1)).max() <= 1e-12
    assert acc == float(f15["pose_accuracy"])
    assert abs(med - float(f15["pose_median"])) <= 1e-12


# ---------------------------------------------------------------------------------------------------- the ICP oracle
def test_icp_oracle_recovers_a_known_rotation():
    rng = np.random.default_rng(15)
    tgt = shape_cloud(3000, rng)
    R = rotation([0.3, -1.0, 0.5], 0.35)
    t = np.array([0.02, -0.03, 0.01])
    src = (tgt[rng.permutation(3000)[:1500]] - t) @ R   # src = R^T (q - t): the true transform maps src back to tgt
    T, fit, rmse, it = icp_oracle(src, tgt, 0.2, max_iteration=100)
    assert np.abs(T[:3, :3] - R).max() < 1e-6 and np.abs(T[:3, 3] - t).max() < 1e-6
    assert fit == 1.0 and rmse < 1e-6 and 1 < it < 100


def test_icp_oracle_semantics_edge_cases():
    rng = np.random.default_rng(16)
    tgt = rng.uniform(-0.5, 0.5, size=(200, 3))
    # no inlier: identity, fitness 0, converged after one (identity) update
    T, fit, rmse, it = icp_oracle(tgt + 10.0, tgt, 0.2)
    assert np.array_equal(T, np.eye(4)) and fit == 0.0 and rmse == 0.0 and it == 1
    # max_iteration = 0: the initial evaluation only
    T, fit, rmse, it = icp_oracle(tgt[:50] + 0.01, tgt, 0.2, max_iteration=0)
    assert np.array_equal(T, np.eye(4)) and it == 0 and fit == 1.0


# ---------------------------------------------------------------------------------------------------- C ABI, no GPU
def _c(a, dtype=np.int32):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_icp_workspace_bytes():
    from dpc.render import _native

    L = _native.lib()
    sc, psc = _c([10, 300, 0])
    tc, ptc = _c([5, 20000, 7])
    n = L.dpc_icp_workspace_bytes(3, psc, ptc)
    # working cloud + at least one slice of (d2, index) per (pair, source) + moments + per-pair state
    assert n >= 3 * 300 * (3 * 8 + 8 + 4) + 3 * 2 * 17 * 8 + 3 * 32 * 8
    assert n % 16 == 0
    bigger, pb = _c([10, 600, 0])
    assert L.dpc_icp_workspace_bytes(3, pb, ptc) > n
    assert L.dpc_icp_workspace_bytes(0, psc, ptc) == 0
    neg, pn = _c([10, -1, 0])
    assert L.dpc_icp_workspace_bytes(3, pn, ptc) == 0


@pytest.mark.parametrize("case", ["ok", "max_dist0", "max_dist_neg", "max_dist_nan", "max_dist_inf", "max_iter_neg",
                                  "neg_count", "neg_start", "src_range", "tgt_range", "empty_target"])
def test_icp_argument_checks_come_before_any_launch(case):
    """With NULL device pointers a valid call gets as far as DPC_ERR_NULL: every DPC_ERR_SHAPE below is returned before
    the library looks at a device pointer or launches anything."""
    from dpc.render import _native

    L = _native.lib()
    desc = [[0, 10, 0, 5], [10, 20, 5, 7]]
    md, mi, n_src, n_tgt = 0.2, 30, 30, 12
    if case == "max_dist0":
        md = 0.0
    elif case == "max_dist_neg":
        md = -0.2
    elif case == "max_dist_nan":
        md = float("nan")
    elif case == "max_dist_inf":
        md = float("inf")
    elif case == "max_iter_neg":
        mi = -1
    elif case == "neg_count":
        desc[1][1] = -1
    elif case == "neg_start":
        desc[1][2] = -5
    elif case == "src_range":
        n_src = 29
    elif case == "tgt_range":
        desc[1][2] = 6
    elif case == "empty_target":
        desc[0][3] = 0
    d, pd = _c(desc)
    rc = L.dpc_icp_point_to_point(None, n_src, None, n_tgt, None, pd, 2, None, md, mi, 1e-6, 1e-6,
                                  None, None, None, None, None, None)
    if case == "ok":
        assert rc == -1   # DPC_ERR_NULL: the arguments passed, the missing buffers stop it
    else:
        assert rc == _native.DPC_ERR_SHAPE


def test_icp_python_refuses_bad_arguments_without_a_device():
    from dpc.render import icp_point_to_point

    a = np.zeros((4, 3))
    for kw in (dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("nan")),
               dict(max_correspondence_distance=0.2, max_iteration=-1)):
        with pytest.raises(ValueError):
            icp_point_to_point([a], [a], **kw)
    with pytest.raises(ValueError):
        icp_point_to_point([a], [np.zeros((0, 3))], 0.2)
    with pytest.raises(ValueError):
        icp_point_to_point([np.zeros((4, 2))], [a], 0.2)
