"""Alignment of unsupervised predictions to the ground-truth frame, and the pose-accuracy metric.

An unsupervised run learns its shapes in a canonical frame of its own.  The reference finds one global rotation to the
ground-truth frame (dpc/run/compute_alignment.py): per validation model and view an ICP of the predicted cloud against
the GT cloud, started from conj(q_gt) * q_pred, then a selection of the best views and models by inlier RMSE and
Markley's quaternion average.  That rotation is the `reference_rotation` of chamfer_of_predictions (eval_chamfer_to.py,
eval_unsupervised_shape) and of pose_errors (eval_camera_pose_to.py).

The ICP runs on the GPU (csrc/dpc_icp.hip, all pairs in one call) with the semantics of open3d 0.9's point-to-point
registration_icp; the rest is host code in fp64 numpy that restates the reference's functions op for op.  Reading and
writing .mat files stays with the caller: everything here takes and returns arrays.
"""
import math

import numpy as np
import torch

from . import _batch, _native

ICP_THRESHOLD = 0.2  # compute_alignment.py:37


# ------------------------------------------------------------------------------------------------------
# batched ICP                                             reference: compute_alignment.py:28-42 (open3d_icp)
# ------------------------------------------------------------------------------------------------------
# Host numpy rather than _batch.cloud's tensors: ICP packs its clouds on the host, and the round trip through torch
# cost a 250-pair call about 1.5 ms.
def _as_f64_cloud(x, what, i):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s[%d] must be [n,3], got %s" % (what, i, tuple(a.shape)))
    return np.ascontiguousarray(a, dtype=np.float64)   # float32 -> float64 is exact, like open3d's Vector3dVector


def icp_point_to_point(sources, targets, max_correspondence_distance, init=None, max_iteration=30, relative_fitness=1e-6,
                       relative_rmse=1e-6, target_of=None):
    """Point-to-point ICP of every sources[i] against targets[target_of[i]], all pairs in one GPU call (fp64).

    Semantics of open3d 0.9's registration_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationPointToPoint(), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)); see
    include/dpc_render.h (dpc_icp_point_to_point).  sources, targets: lists of [n,3] tensors or arrays; target_of: one
    target index per source (default: i -> i), so views of one model can share their GT cloud; init: [P,4,4] or [4,4]
    (default identity).  Returns (transform [P,4,4], fitness [P], inlier_rmse [P], iterations [P]) on the GPU: fp64, and
    iterations (the number of updates applied) int32.  Bad arguments raise ValueError before anything is launched."""
    srcs = [_as_f64_cloud(s, "sources", i) for i, s in enumerate(sources)]
    tgts = [_as_f64_cloud(t, "targets", i) for i, t in enumerate(targets)]
    P = len(srcs)
    if target_of is None:
        if len(tgts) != P:
            raise ValueError("icp_point_to_point: %d sources and %d targets need target_of" % (P, len(tgts)))
        target_of = range(P)
    target_of = [int(k) for k in target_of]
    if len(target_of) != P or any(k < 0 or k >= len(tgts) for k in target_of):
        raise ValueError("icp_point_to_point: target_of must map each of the %d sources to one of %d targets" % (P, len(tgts)))
    if init is None:
        init_np = np.broadcast_to(np.eye(4), (P, 4, 4))
    else:
        init_np = init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
        if init_np.shape == (4, 4):
            init_np = np.broadcast_to(init_np, (P, 4, 4))
        if init_np.shape != (P, 4, 4):
            raise ValueError("icp_point_to_point: init must be [4,4] or [%d,4,4], got %s" % (P, tuple(init_np.shape)))
    init_np = np.ascontiguousarray(init_np, dtype=np.float64)

    src_start = np.cumsum([0] + [len(s) for s in srcs])
    tgt_start = np.cumsum([0] + [len(t) for t in tgts])
    L = _native.lib()
    n_src, n_tgt = int(src_start[-1]), int(tgt_start[-1])
    if n_src > _batch.INT32_MAX or n_tgt > _batch.INT32_MAX:
        raise ValueError("icp_point_to_point: more than 2^31 - 1 points")
    desc = _batch.table([(src_start[i], len(srcs[i]), tgt_start[k], len(tgts[k])) for i, k in enumerate(target_of)], 4,
                        "icp_point_to_point: more than 2^31 - 1 points")
    host_desc = desc.ctypes.data
    _batch.dry_run(L.dpc_icp_point_to_point(None, n_src, None, n_tgt, None, host_desc, P, None,
                                            float(max_correspondence_distance), int(max_iteration),
                                            float(relative_fitness), float(relative_rmse), None, None, None, None, None,
                                            None),
                   "icp_point_to_point: invalid arguments (max_correspondence_distance %r, max_iteration %r, an empty "
                   "target for a non-empty source, or a range outside the clouds)"
                   % (max_correspondence_distance, max_iteration))
    dev = _batch.device("dpc.render.icp_point_to_point", sources, targets,
                        [init] if isinstance(init, torch.Tensor) else [])
    out_t = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    out_f = torch.empty((P,), dtype=torch.float64, device=dev)
    out_r = torch.empty((P,), dtype=torch.float64, device=dev)
    out_i = torch.empty((P,), dtype=torch.int32, device=dev)
    if P == 0:
        return out_t, out_f, out_r, out_i
    src = torch.from_numpy(np.concatenate(srcs) if n_src else np.zeros((1, 3))).to(dev)
    tgt = torch.from_numpy(np.concatenate(tgts) if n_tgt else np.zeros((1, 3))).to(dev)
    desc_d = _batch.on_device(desc, dev)
    init_d = torch.from_numpy(init_np).to(dev)
    counts = np.ascontiguousarray(desc[:, 1]), np.ascontiguousarray(desc[:, 3])
    ws = _batch.workspace(L.dpc_icp_workspace_bytes(P, counts[0].ctypes.data, counts[1].ctypes.data), dev)
    _native.call(dev, "dpc_icp_point_to_point", _native.ptr(src), n_src, _native.ptr(tgt), n_tgt, _native.ptr(desc_d), host_desc, P,
                 _native.ptr(init_d), float(max_correspondence_distance), int(max_iteration), float(relative_fitness),
                 float(relative_rmse), _native.ptr(out_t), _native.ptr(out_f), _native.ptr(out_r), _native.ptr(out_i),
                 _native.ptr(ws))
    return out_t, out_f, out_r, out_i


# ------------------------------------------------------------------------------------------------------
# host helpers, fp64 numpy      reference: util/quaternion.py:189-240, util/camera.py:46-59, util/euler.py
# ------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    """quaternion_multiply(_np), elementwise over [..., 4] in the reference's term order."""
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w2, x2, y2, z2 = (b[..., k] for k in range(4))
    w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    y = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2
    z = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2
    return np.stack([w, x, y, z], axis=-1)


_CONJ = np.array([1.0, -1.0, -1.0, -1.0])


def _normalise(q):
    return q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))


def as_rotation_matrix(q):
    """util/quaternion.py:189-212: [..., 4] (w, x, y, z), normalised first -> [..., 3, 3]."""
    q = _normalise(np.asarray(q, dtype=np.float64))
    w, x, y, z = (q[..., k] for k in range(4))

    def diag(a, b):
        return 1 - 2 * a ** 2 - 2 * b ** 2

    def tr_add(a, b, c, d):
        return 2 * a * b + 2 * c * d

    def tr_sub(a, b, c, d):
        return 2 * a * b - 2 * c * d

    m = [[diag(y, z), tr_sub(x, y, z, w), tr_add(x, z, y, w)],
         [tr_add(x, y, z, w), diag(x, z), tr_sub(y, z, x, w)],
         [tr_sub(x, z, y, w), tr_add(y, z, x, w), diag(x, y)]]
    return np.stack([np.stack(m[i], axis=-1) for i in range(3)], axis=-2)


def from_rotation_matrix(mtr):
    """util/quaternion.py:215-240: [..., 3, 3] -> [..., 4] with w = sqrt(1 + tr) / 2.  NaN where 1 + tr < 0 (rotations
    near 180 degrees), exactly where the reference's is; its selection step drops those rows."""
    m = np.asarray(mtr, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.sqrt(1.0 + m[..., 0, 0] + m[..., 1, 1] + m[..., 2, 2]) / 2
        x = (m[..., 2, 1] - m[..., 1, 2]) / (4 * w)
        y = (m[..., 0, 2] - m[..., 2, 0]) / (4 * w)
        z = (m[..., 1, 0] - m[..., 0, 1]) / (4 * w)
    return np.stack([w, x, y, z], axis=-1)


def _axis_angle_quaternion(angle, axis):
    c = math.cos(angle / 2)
    s = math.sin(angle / 2)
    q = np.zeros(4)
    q[0] = c
    q[1:4] = s * np.asarray(axis)
    return q


def quaternion_from_campos(cam_pos):
    """util/camera.py:46-59 with util/euler.py's ypr_from_campos and quaternionFromYawPitchRoll, in fp64."""
    cx, cy, cz = (float(v) for v in np.asarray(cam_pos, dtype=np.float64).reshape(3))
    cam_dist = math.sqrt(cx * cx + cy * cy + cz * cz)
    cx, cy, cz = cx / cam_dist, cy / cam_dist, cz / cam_dist
    t = math.sqrt(cx * cx + cy * cy)
    tx, ty = cx / t, cy / t
    yaw = math.acos(tx)
    if ty > 0:
        yaw = 2 * math.pi - yaw
    pitch, roll = math.asin(cz), 0
    yaw = yaw + math.pi
    q_yaw = _axis_angle_quaternion(yaw, np.array([0, 1, 0]))
    q_pitch = _axis_angle_quaternion(pitch, np.array([0, 0, 1]))
    q_roll = _axis_angle_quaternion(roll, np.array([1, 0, 0]))
    return _qmul(q_roll, _qmul(q_pitch, q_yaw))


# ------------------------------------------------------------------------------------------------------
# alignment                                        reference: compute_alignment.py:45-127, 130-181
# ------------------------------------------------------------------------------------------------------
def _unrotation(quat_pred, quat_gt):
    """conj(normalise(q_gt)) * normalise(q_pred) ([..., 4] each), compute_alignment.py:66-71."""
    qp = _normalise(np.asarray(quat_pred, dtype=np.float64))
    qg = _normalise(np.asarray(quat_gt, dtype=np.float64))
    return _qmul(qg * _CONJ, qp)


def _rotation_from_icp(T):
    rot = np.asarray(T, dtype=np.float64)[..., :3, :3]   # the translation is discarded
    det = np.linalg.det(rot)
    assert np.all(np.fabs(det - 1.0) <= 0.0001), det   # compute_alignment.py:77
    return from_rotation_matrix(rot)


def alignment_to_ground_truth(pc_pred, quat_pred, gt_pred, quat_gt):
    """compute_alignment.py:45-82: ICP (threshold 0.2) of the predicted cloud against the GT cloud, started from
    as_rotation_matrix(conj(q_gt) * q_pred) with zero translation.  Returns (quat [1,4] fp64, inlier_rmse)."""
    init = np.eye(4)
    init[:3, :3] = as_rotation_matrix(_unrotation(np.reshape(_host(quat_pred), (1, 4)), np.reshape(_host(quat_gt), (1, 4))))[0]
    T, _, rmse, _ = icp_point_to_point([pc_pred], [gt_pred], ICP_THRESHOLD, init=init[None])
    return _rotation_from_icp(T.cpu().numpy()), float(rmse[0])


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def alignment_candidates(pred_clouds, pred_quats, gt_clouds, gt_quats):
    """compute_alignment_candidates (compute_alignment.py:85-127) for M models x V views in ONE batched ICP call.

    pred_clouds [M][V] clouds [n,3]; pred_quats [M,V,4] predicted camera quaternions; gt_clouds [M] GT clouds (None: no GT
    file for that model); gt_quats [M,V,4] GT camera quaternions (quaternion_from_campos of the views' cam_pos).
    Returns (rotations [M,V,4], rmse [M,V]) float32, as the reference stores them; models without GT keep rmse 1 and a
    zero rotation."""
    pred_quats, gt_quats = _host(pred_quats), _host(gt_quats)
    M = len(pred_clouds)
    V = pred_quats.shape[1] if M else 0
    rmse = np.ones((M, V), np.float32)
    rotations = np.zeros((M, V, 4), np.float32)
    sources, targets, target_of, inits, where = [], [], [], [], []
    for m in range(M):
        if gt_clouds[m] is None:
            continue
        targets.append(gt_clouds[m])
        for v in range(V):
            sources.append(pred_clouds[m][v])
            target_of.append(len(targets) - 1)
            init = np.eye(4)
            init[:3, :3] = as_rotation_matrix(_unrotation(pred_quats[m, v].reshape(1, 4), gt_quats[m, v].reshape(1, 4)))[0]
            inits.append(init)
            where.append((m, v))
    if not sources:
        return rotations, rmse
    T, _, err, _ = icp_point_to_point(sources, targets, ICP_THRESHOLD, init=np.stack(inits), target_of=target_of)
    quats = _rotation_from_icp(T.cpu().numpy())
    err = err.cpu().numpy()
    for k, (m, v) in enumerate(where):
        rmse[m, v] = err[k]
        rotations[m, v, :] = quats[k]
    return rotations, rmse


def quat_w_avg_markley(Q):
    """util/quaternion_average.py quatWAvgMarkley with unit weights: the eigenvector of the largest eigenvalue of
    mean(q q^T) (np.linalg.eig, np.argsort), sign chosen so that w >= 0."""
    Q = np.asarray(Q)
    A = np.zeros((4, 4))
    M = Q.shape[0]
    weights = np.ones(M)
    w_sum = 0
    for i in range(M):
        q = np.expand_dims(Q[i, :], -1)
        A = weights[i] * np.matmul(q, q.transpose()) + A
        w_sum = w_sum + weights[i]
    A = 1.0 / w_sum * A
    w, v = np.linalg.eig(A)
    q_avg = v[:, np.argsort(w)[-1]]
    if q_avg[0] < -0:
        q_avg *= -1.0
    return q_avg


def reference_rotation(rotations, rmse, num_filtered=2, num_to_estimate=15):
    """compute_alignment.py:147-176: per model the num_filtered views of lowest rmse, the num_to_estimate models of lowest
    mean of those, NaN rows dropped, Markley's average of the rest.  Returns the rotation quaternion [4]."""
    rotations, rmse = np.asarray(rotations), np.asarray(rmse)
    num_models = rotations.shape[0]
    rotations_filtered = np.zeros((num_models, num_filtered, 4))
    rmse_filtered = np.zeros((num_models, num_filtered))
    for model_idx in range(num_models):
        rmse_m = rmse[model_idx, :]
        indices = np.argsort(rmse_m)[0:num_filtered]
        rmse_filtered[model_idx, :] = rmse_m[indices]
        rotations_filtered[model_idx, :, :] = rotations[model_idx, indices, :]
    model_mean_rmse = np.mean(rmse_filtered, axis=1)
    models_indices = np.argsort(model_mean_rmse)[0:num_to_estimate]
    reference_rotations = np.reshape(rotations_filtered[models_indices, :, :], [-1, 4])
    good = np.logical_not(np.any(np.isnan(reference_rotations), axis=1))
    return quat_w_avg_markley(reference_rotations[good, :])


# ------------------------------------------------------------------------------------------------------
# pose accuracy                                     reference: eval_camera_pose_to.py:17-20, 45-88
# ------------------------------------------------------------------------------------------------------
def pose_errors(pred_quats, gt_cam_pos, reference_rotation, threshold_deg=30):
    """Angle error of every predicted camera after the global alignment, as run_eval computes it: aligned = q_pred / |q_pred|
    * conj(reference_rotation), error = |2 arccos(w(conj(q_gt) * aligned))| wrapped into [0, pi].
    pred_quats [N,4], gt_cam_pos [N,3] (one row per view, models concatenated), reference_rotation [4] or [1,4].
    Returns (angle_error [N] radians, accuracy = share below threshold_deg, median error in degrees)."""
    pred = np.array(_host(pred_quats), dtype=np.float64).reshape(-1, 4)
    cam = np.asarray(_host(gt_cam_pos), dtype=np.float64).reshape(-1, 3)
    ref_conj = np.asarray(reference_rotation, dtype=np.float64).reshape(1, 4) * _CONJ
    errors = np.zeros(len(pred), dtype=np.float64)
    for i in range(len(pred)):
        gt_q = quaternion_from_campos(cam[i])
        q = pred[i] / np.linalg.norm(pred[i])
        aligned = _qmul(q, ref_conj[0])
        q_diff = _qmul(gt_q * _CONJ, aligned)
        with np.errstate(invalid="ignore"):
            ang = 2 * np.arccos(q_diff[0])
        if ang > np.pi:
            ang -= 2 * np.pi
        errors[i] = np.fabs(ang)
    correct = errors < threshold_deg / 180.0 * np.pi
    n = correct.shape[0]
    accuracy = np.count_nonzero(correct) / n
    median = np.sort(errors)[n // 2] / np.pi * 180
    return errors, accuracy, median
