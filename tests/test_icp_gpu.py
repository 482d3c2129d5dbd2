"""GPU tests of the batched ICP (csrc/dpc_icp.hip through dpc.render.icp_point_to_point) and the alignment pipeline built on
it, against the fp64 oracle of tests/test_alignment_host.py (open3d 0.9's point-to-point semantics) and against the nearest
kernel already pinned by F11.  Each test is a fresh, small launch."""
import numpy as np
import pytest
import torch

from test_alignment_host import icp_oracle, rotation, shape_cloud

pytestmark = pytest.mark.gpu

TAU = 0.2


def _dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _ragged_batch(rng):
    """12 pairs: n_src 1 .. 9000, n_tgt 1 .. 20000, shared targets, outliers beyond tau, a pair without inliers, a pair that
    converges after one update and pairs that run into max_iteration."""
    big = shape_cloud(20000, rng)
    mid = shape_cloud(1025, rng)
    small = rng.uniform(-0.3, 0.3, size=(300, 3))
    one = np.array([[0.05, -0.02, 0.1]])
    targets = [big, mid, small, one]

    def moved(pts, axis, angle, t, noise):
        return (pts - t) @ rotation(axis, angle) + rng.normal(size=pts.shape) * noise

    sources, target_of, inits = [], [], []

    def add(src, k, init=None):
        sources.append(src)
        target_of.append(k)
        inits.append(np.eye(4) if init is None else init)

    add(moved(big[rng.permutation(20000)[:9000]], [1, 2, 3], 0.3, [0.03, 0, 0.02], 0.005), 0)     # large, slow
    add(moved(big[rng.permutation(20000)[:3000]], [0, 1, 0], 0.15, [0, 0.02, 0], 0.002), 0)       # shares target 0
    far = rng.uniform(-0.5, 0.5, size=(400, 3)) + [2.0, 0, 0]                                     # outliers beyond tau
    add(np.concatenate([moved(mid[:600], [1, 0, 1], 0.1, [0.01, 0.01, 0], 0.003), far]), 1)
    add(small[:257].copy(), 2)                                                                    # exact subset: 1 update
    add(small[:40] + 10.0, 2)                                                                     # no inlier at all
    add(rng.normal(size=(1, 3)) * 0.05, 3)                                                        # n_src = 1, n_tgt = 1
    add(rng.uniform(-0.2, 0.2, size=(50, 3)), 3)                                                  # 1 target, partial inliers
    init = np.eye(4)
    init[:3, :3] = rotation([0, 0, 1], 0.4)
    add(moved(mid, [0, 0, 1], 0.45, [0, 0, 0], 0.004), 1, init)                                   # init close to the truth
    add(moved(small[:299], [1, -1, 0], 0.2, [0.02, 0, 0], 0.01), 2)
    add(moved(big[:5000], [2, 1, 0], 0.5, [0, 0, 0.05], 0.003), 0)                                # 30 deg: may not converge
    add(moved(mid[:256], [0, 1, 1], 0.05, [0, 0, 0], 0.0), 1)
    add(moved(big[7000:7700], [1, 1, 1], 0.25, [0.01, 0.01, 0.01], 0.02), 0)
    return sources, targets, target_of, np.stack(inits)


def test_ragged_batch_matches_the_oracle():
    import dpc.render as R

    rng = np.random.default_rng(150)
    sources, targets, target_of, inits = _ragged_batch(rng)
    max_it = 12
    T, fit, rmse, it = (x.cpu().numpy() for x in R.icp_point_to_point(sources, targets, TAU, init=inits,
                                                                         max_iteration=max_it, target_of=target_of))
    iters = []
    worst_t = 0.0
    for p, src in enumerate(sources):
        To, fo, ro, io = icp_oracle(src, targets[target_of[p]], TAU, init=inits[p], max_iteration=max_it)
        iters.append(io)
        assert it[p] == io, (p, it[p], io)
        assert round(fit[p] * len(src)) == round(fo * len(src)) and fit[p] == fo, (p, fit[p], fo)
        # relative, plus 1e-15 absolute for the zero-residual pair: there the two solvers' last-ulp differences in R (Horn's
        # eigenvector here, an SVD in the oracle) are all of inlier_rmse (measured: 0 here against 9.1e-17)
        assert abs(rmse[p] - ro) <= 1e-12 * ro + 1e-15, (p, rmse[p], ro)
        assert np.abs(np.linalg.det(T[p][:3, :3]) - 1) < 1e-12
        if len(targets[target_of[p]]) == 1:
            # every inlier pairs with the one target point: Sigma is zero and the rotation undetermined.  The kernel's
            # anchored moments give exactly zero, hence the identity; the oracle's SVD (like open3d's Eigen SVD) turns the
            # rounding of the centroid into an arbitrary rotation (0.82 here).  The distances to one point do not depend on
            # it, so iterations, fitness and rmse are still compared above.
            assert np.array_equal(T[p][:3, :3], np.eye(3)), (p, T[p])
            continue
        worst_t = max(worst_t, np.abs(T[p] - To).max())
    print("worst |T - T_oracle| = %.3e, iterations %s" % (worst_t, iters))
    assert worst_t <= 1e-13   # measured 3.1e-15: the two solvers differ in the last bits of R and t only
    assert iters[3] == 1 and iters[4] == 1 and max_it in iters   # the exact subset, the pair without inliers, a capped pair
    assert fit[4] == 0.0 and rmse[4] == 0.0 and np.array_equal(T[4], np.eye(4))


def test_initial_evaluation_matches_the_nearest_kernel():
    import dpc.render as R

    dev = _dev()
    rng = np.random.default_rng(151)
    for ns, nt in ((1, 1), (700, 3000), (4100, 1300)):
        src = rng.uniform(-0.6, 0.6, size=(ns, 3))
        tgt = rng.uniform(-0.6, 0.6, size=(nt, 3))
        _, fit, rmse, it = R.icp_point_to_point([src], [tgt], TAU, max_iteration=0)
        _, dist, _ = R.point_cloud_distance(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev))
        dist = dist.cpu().numpy()
        inl = dist < TAU
        assert int(it[0]) == 0
        assert fit[0].item() * ns == inl.sum()
        if inl.any():
            ref = np.sqrt(np.mean(dist[inl] ** 2))
            assert abs(rmse[0].item() - ref) <= 1e-14 * ref
        else:
            assert rmse[0].item() == 0.0


def test_two_identical_calls_are_bit_identical():
    import dpc.render as R

    rng = np.random.default_rng(152)
    sources, targets, target_of, inits = _ragged_batch(rng)
    a = R.icp_point_to_point(sources, targets, TAU, init=inits, max_iteration=6, target_of=target_of)
    b = R.icp_point_to_point(sources, targets, TAU, init=inits, max_iteration=6, target_of=target_of)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def test_end_to_end_alignment_recovers_a_hidden_rotation():
    import dpc.render as R
    from dpc.render import alignment as A

    dev = _dev()
    rng = np.random.default_rng(153)
    M, V, noise = 6, 5, 0.004
    q_h = _quat([0.4, 1.0, -0.3], 1.1)   # hidden global rotation: prediction frame -> GT frame
    R_h = R.as_rotation_matrix(q_h[None])[0]
    gt_clouds, pred_clouds, pred_quats, gt_quats, cam_pos = [], [], np.zeros((M, V, 4)), np.zeros((M, V, 4)), np.zeros((M, V, 3))
    for m in range(M):
        gt = shape_cloud(2500, rng) * rng.uniform(0.8, 1.2, size=3)
        gt_clouds.append(gt)
        views = []
        for v in range(V):
            pred = gt[rng.permutation(len(gt))[:2000]] @ R_h + rng.normal(size=(2000, 3)) * noise   # R_h^T q + noise
            views.append(torch.from_numpy(pred.astype(np.float32)))
            cam_pos[m, v] = rng.normal(size=3) * 2
            gt_quats[m, v] = R.quaternion_from_campos(cam_pos[m, v])
            err = _quat(rng.normal(size=3), rng.uniform(0, 0.25))   # camera error up to ~14 degrees
            pred_quats[m, v] = A._qmul(A._qmul(gt_quats[m, v], q_h), err) * rng.uniform(0.5, 2.0)
        pred_clouds.append(views)
    rotations, rmse = R.alignment_candidates(pred_clouds, pred_quats, gt_clouds, gt_quats)
    assert rotations.dtype == np.float32 and rmse.dtype == np.float32 and rmse.shape == (M, V)
    q_ref = R.reference_rotation(rotations, rmse)
    ang = 2 * np.arccos(min(1.0, abs(float(np.dot(q_ref, q_h)))))
    assert ang < 1e-3, ang

    # the same pipeline with the oracle in place of the kernel
    rot_o, rmse_o = np.zeros((M, V, 4), np.float32), np.zeros((M, V), np.float32)
    for m in range(M):
        for v in range(V):
            init = np.eye(4)
            init[:3, :3] = R.as_rotation_matrix(A._unrotation(pred_quats[m, v][None], gt_quats[m, v][None]))[0]
            To, _, ro, _ = icp_oracle(pred_clouds[m][v].double().numpy(), gt_clouds[m], TAU, init=init)
            rot_o[m, v], rmse_o[m, v] = A._rotation_from_icp(To[None])[0], ro
    assert np.array_equal(rmse, rmse_o) or np.abs(rmse - rmse_o).max() <= 1e-6 * rmse_o.max()
    assert np.abs(q_ref - R.reference_rotation(rot_o, rmse_o)).max() <= 1e-9

    # with the rotation the Chamfer distance drops to the noise level; without it it does not
    pts = [np.stack([c.numpy() for c in views]) for views in pred_clouds]
    aligned = np.concatenate([R.chamfer_of_predictions(pts[m], gt_clouds[m], q_ref[None], device=dev) for m in range(M)])
    raw = np.concatenate([R.chamfer_of_predictions(pts[m], gt_clouds[m], None, device=dev) for m in range(M)])
    assert aligned.max() < 0.03 < raw.min(), (aligned.max(), raw.min())

    err, acc, med = R.pose_errors(pred_quats.reshape(-1, 4), cam_pos.reshape(-1, 3), q_ref)
    assert acc == 1.0 and med < 15.0


@pytest.mark.parametrize("case", ["max_dist0", "max_dist_nan", "max_dist_inf", "max_iter_neg", "empty_target"])
def test_bad_arguments_raise_before_any_launch(case):
    import dpc.render as R
    from dpc.render import _native
    from dpc.render._ops import status_word

    dev = _dev()
    a = torch.rand(64, 3, dtype=torch.float64, device=dev)
    kw = dict(max_correspondence_distance=TAU)
    targets = [a]
    if case == "max_dist0":
        kw["max_correspondence_distance"] = 0.0
    elif case == "max_dist_nan":
        kw["max_correspondence_distance"] = float("nan")
    elif case == "max_dist_inf":
        kw["max_correspondence_distance"] = float("inf")
    elif case == "max_iter_neg":
        kw["max_iteration"] = -1
    elif case == "empty_target":
        targets = [a[:0]]
    raised = []

    def call():
        try:
            R.icp_point_to_point([a], targets, **kw)
        except ValueError as e:
            raised.append(e)

    launched = _native.launched_instantiations(call, dev)
    assert raised and launched == set()
    torch.cuda.synchronize(dev)
    assert int(status_word(dev).item()) == 0
