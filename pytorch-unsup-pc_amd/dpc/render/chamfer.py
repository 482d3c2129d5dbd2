"""The Chamfer half of the evaluation for a whole split in batched GPU calls (dpc/run/eval_chamfer_to.py:88-145).

The reference walks models and views one at a time: per view two compute_distance calls (pred -> GT, GT -> pred) and
np.mean of each float64 result.  Here every directed pair of a group of models goes into one dpc_nearest_batched call
(csrc/dpc_chamfer.hip): the nearest search is dpc_point_cloud_distance's, and the per-pair means are summed on the device
in numpy's float64 order, so every number equals the reference's own compute_distance + np.mean bit for bit.

    nearest_batched   the thin wrapper over the C ABI: packed points, a [P,4] pair table, [P] float64 means
    chamfer_batched   (mean pred -> gt, mean gt -> pred) for lists of clouds, [P,2] float64
    chamfer_loss      the same two means as a differentiable loss (optionally of squared distances): gradients reach
                      every prediction and GT cloud that requires them (csrc/dpc_chamfer_bwd.hip)
    chamfer_of_split  the reference's chamfer_dists [M,V,2] for loaded predictions and GT clouds
    eval_chamfer      run_eval's file loop: <save_dir>/<model>_pc.pkl plus a caller-supplied GT loader

Reading .mat files stays with the caller (load_gt), as everywhere in this package.
"""
import os

import numpy as np
import torch

from . import _batch, _native, _split
from .predictions import load_predictions

_WHAT = "dpc.render Chamfer evaluation"


def _pair_table(pairs):
    desc = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if desc.ndim != 2 or desc.shape[1] != 4:
        raise ValueError("nearest_batched: pairs must be [P,4] (src_start, src_count, tgt_start, tgt_count), got %s"
                         % (tuple(desc.shape),))
    return _batch.table(desc, 4, "nearest_batched: pair table entries must fit int32")


def _forward(pts, desc, dev, dtype, want_points, squared):
    """One dpc_nearest_batched call on pts (on dev, in dtype, contiguous): (means, values, min_dist, idx, device table);
    values are the distances, or their squares (rounded once) with `squared`, whose means then come from
    dpc_chamfer_pair_means, the same summation kernels.  Without want_points the last four are None."""
    L = _native.lib()
    P, n_pts = desc.shape[0], int(pts.shape[0])
    is64 = int(dtype == torch.float64)
    host_desc = desc.ctypes.data
    total = int(desc[:, 1].astype(np.int64).sum()) if P else 0
    mean = torch.empty((P,), dtype=torch.float64, device=dev)
    dist = torch.empty((total,), dtype=dtype, device=dev) if want_points else None
    idx = torch.empty((total,), dtype=torch.int64, device=dev) if want_points else None
    val, desc_d = dist, None
    if P:
        desc_d = _batch.on_device(desc, dev)
        ws = _batch.workspace(L.dpc_chamfer_workspace_bytes(P, host_desc, is64), dev)
        _native.call(dev, "dpc_nearest_batched", _native.ptr(pts), n_pts, is64, _native.ptr(desc_d), host_desc, P,
                     _native.ptr(mean), _native.ptr(dist), _native.ptr(idx), _native.ptr(ws))
        if squared:
            val = dist * dist
            _native.call(dev, "dpc_chamfer_pair_means", _native.ptr(val), is64, _native.ptr(desc_d), host_desc, P,
                         _native.ptr(mean), _native.ptr(ws))
    elif squared:
        val = dist * dist
    return mean, val, dist, idx, desc_d


class _NearestBatched(torch.autograd.Function):
    """nearest_batched with a gradient: the forward keeps the packed points, the table and its own min_dist / idx, the
    backward is one dpc_nearest_batched_bwd call (csrc/dpc_chamfer_bwd.hip)."""

    @staticmethod
    def forward(ctx, points, desc, dev, dtype, squared):
        pts = points.detach().to(device=dev, dtype=dtype).contiguous()
        mean, val, dist, idx, desc_d = _forward(pts, desc, dev, dtype, True, squared)
        ctx.save_for_backward(pts, dist, idx)
        ctx.desc, ctx.desc_d, ctx.squared, ctx.like = desc, desc_d, bool(squared), (points.device, points.dtype)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(idx)
        return mean, val, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gmean, gval, _gidx):
        pts, dist, idx = ctx.saved_tensors
        desc, dev, dtype = ctx.desc, pts.device, pts.dtype
        P, n_pts, is64 = desc.shape[0], int(pts.shape[0]), int(pts.dtype == torch.float64)
        if P == 0 or (gmean is None and gval is None):
            dpts = torch.zeros_like(pts)
        else:
            L = _native.lib()
            host_desc = desc.ctypes.data
            gmean = None if gmean is None else gmean.to(device=dev, dtype=torch.float64).contiguous()
            gval = None if gval is None else gval.to(device=dev, dtype=dtype).contiguous()
            dpts = torch.empty_like(pts)
            ws = _batch.workspace(L.dpc_chamfer_bwd_workspace_bytes(P, host_desc, is64), dev)
            _native.call(dev, "dpc_nearest_batched_bwd", _native.ptr(pts), n_pts, is64, _native.ptr(ctx.desc_d), host_desc, P,
                         _native.ptr(dist), _native.ptr(idx), _native.ptr(gmean), _native.ptr(gval), int(ctx.squared),
                         _native.ptr(dpts), _native.ptr(ws))
        return dpts.to(device=ctx.like[0], dtype=ctx.like[1]), None, None, None, None


def nearest_batched(points, pairs, return_distances=False, squared=False):
    """Nearest-target distances of P directed pairs over one packed cloud buffer, with per-pair float64 means.

    points: [n,3] tensor (or array) holding every cloud; pairs: [P,4] rows (src_start, src_count, tgt_start, tgt_count)
    indexing it.  Pair p's distances are exactly point_cloud_distance(points[src], points[tgt])[1] and its mean is
    np.mean of them as float64, bit for bit (NaN when src_count == 0).  fp64 arithmetic when points is fp64, fp32
    otherwise (as point_cloud_distance).  Returns means [P] float64 on the device, or (means, min_dist [sum src_count],
    idx [sum src_count] int64) with return_distances, the distances packed in pair order.  With squared, the per-point
    values are the squared distances (d * d, rounded once) and the means are theirs, in the same summation order.  A bad
    table raises ValueError before anything is launched.

    When points requires grad, the means and the per-point values carry gradient (dpc_nearest_batched_bwd; idx does
    not), which arrives in the dtype of points.  The gradient follows idx through ties; where a source coincides with
    its target (distance 0) the reference's autograd gives NaN and this gives exactly zero (include/dpc_render.h)."""
    desc = _pair_table(pairs)
    P = desc.shape[0]
    L = _native.lib()
    pts = _batch.cloud(points, "nearest_batched: points")
    n_pts = int(pts.shape[0])
    if n_pts > _batch.INT32_MAX:
        raise ValueError("nearest_batched: more than 2^31 - 1 points")
    host_desc = desc.ctypes.data
    _batch.dry_run(L.dpc_nearest_batched(None, n_pts, 0, None, host_desc, P, None, None, None, None, None),
                   "nearest_batched: invalid pair table (a negative start or count, a range outside the %d points, "
                   "an empty target for a non-empty source, or more than 2^31 - 1 output points)" % n_pts)
    dev = _batch.device(_WHAT, [pts])
    dtype = torch.float64 if pts.dtype == torch.float64 else torch.float32
    if isinstance(points, torch.Tensor) and points.requires_grad and torch.is_grad_enabled():
        _batch.dry_run(L.dpc_nearest_batched_bwd(None, n_pts, 0, None, host_desc, P, None, None, None, None, 0, None, None,
                                                 None),
                       "nearest_batched: more than 2^31 - 1 target points over the pairs of a differentiable call")
        mean, val, idx = _NearestBatched.apply(points, desc, dev, dtype, bool(squared))
        return (mean, val, idx) if return_distances else mean
    pts = pts.to(device=dev, dtype=dtype).contiguous()
    mean, val, _, idx, _ = _forward(pts, desc, dev, dtype, return_distances or squared, squared)
    return (mean, val, idx) if return_distances else mean


def chamfer_batched(preds, gts, gt_of=None):
    """(mean_i min_j |pred_i - gt_j|, mean_j min_i |gt_j - pred_i|) for every prediction against its GT cloud: the
    reference's chamfer_dists_current rows (eval_chamfer_to.py:119-123), [P,2] float64 on the device.

    preds, gts: lists of [n,3] tensors or arrays; gt_of: the GT index of each prediction (default i -> i), so views of
    one model share one GT copy.  A pair is computed in fp64 when its prediction or its GT is fp64, in fp32 otherwise
    (point_cloud_distance's rule, per pair): all 2P directed pairs go into one native call, or two when fp32-only and
    fp64 pairs are mixed.  NaN or inf coordinates raise ValueError naming the first bad input (one device reduction),
    standing in for the reference's assert on NaN distances; an empty GT for a non-empty prediction raises too."""
    P_list = [_batch.cloud(p, "preds[%d]" % i) for i, p in enumerate(preds)]
    G_list = [_batch.cloud(g, "gts[%d]" % i) for i, g in enumerate(gts)]
    P = len(P_list)
    if gt_of is None:
        if len(G_list) != P:
            raise ValueError("chamfer_batched: %d predictions and %d GT clouds need gt_of" % (P, len(G_list)))
        gt_of = range(P)
    gt_of = list(gt_of)
    if len(gt_of) != P or any(not isinstance(k, (int, np.integer)) or k < 0 or k >= len(G_list) for k in gt_of):
        raise ValueError("chamfer_batched: gt_of must map each of the %d predictions to one of %d GT clouds" % (P, len(G_list)))
    gt_of = [int(k) for k in gt_of]
    for i, k in enumerate(gt_of):
        if len(G_list[k]) == 0 and len(P_list[i]) > 0:
            raise ValueError("chamfer_batched: GT cloud %d is empty but prediction %d is not (argmin of an empty set)" % (k, i))
    dev = _batch.device(_WHAT, P_list, G_list)
    out = torch.empty((P, 2), dtype=torch.float64, device=dev)
    if P == 0:
        return out
    f64 = [P_list[i].dtype == torch.float64 or G_list[k].dtype == torch.float64 for i, k in enumerate(gt_of)]
    for want in (False, True):
        sel = [i for i in range(P) if f64[i] == want]
        if sel:
            out[sel] = _chamfer_group([P_list[i] for i in sel], G_list, [gt_of[i] for i in sel], dev,
                                      torch.float64 if want else torch.float32)
    return out


def _chamfer_group(preds, gts, gt_of, dev, dtype):
    """One native call: the GT clouds used, then the predictions, packed into one buffer; pairs (p->g, g->p) interleaved."""
    used = sorted(set(gt_of))
    clouds = [gts[k] for k in used] + list(preds)
    names = ["gts[%d]" % k for k in used] + ["preds[%d]" % i for i in range(len(preds))]
    packed, start = _batch.pack(clouds, dev, dtype)
    if packed.numel() and not bool(torch.isfinite(packed).all()):
        for name, c in zip(names, clouds):
            if not bool(torch.isfinite(c).all()):
                raise ValueError("chamfer_batched: %s holds a NaN or inf coordinate" % name)
    slot = {k: j for j, k in enumerate(used)}
    desc = np.zeros((2 * len(preds), 4), dtype=np.int64)
    for i, k in enumerate(gt_of):
        ps, pn = start[len(used) + i], len(preds[i])
        gs, gn = start[slot[k]], len(gts[k])
        desc[2 * i] = (ps, pn, gs, gn)
        desc[2 * i + 1] = (gs, gn, ps, pn)
    if start[-1] > _batch.INT32_MAX:
        raise ValueError("chamfer_batched: more than 2^31 - 1 points in one call")
    return nearest_batched(packed, desc).view(len(preds), 2)


def _loss_clouds(x, what):
    """x as a list of [n,3] float32 / float64 tensors that keep their autograd history: a [B,N,3] tensor gives its B
    rows, a list gives its entries (arrays wrapped; other dtypes converted to float32)."""
    if isinstance(x, torch.Tensor) and x.dim() == 3:
        x = x.unbind(0)
    out = []
    for i, c in enumerate(x):
        t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("chamfer_loss: %s[%d] must be [n,3], got %s" % (what, i, tuple(t.shape)))
        out.append(t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float32))
    return out


def chamfer_loss(preds, gts, gt_of=None, squared=False):
    """chamfer_batched as a loss: [P,2] float64 (mean pred -> gt, mean gt -> pred) on the device, carrying gradient to
    every prediction and GT cloud that requires it.  squared: means of the squared distances instead.

    preds, gts: lists of [n,3] tensors or arrays, or [B,N,3] tensors; gt_of as in chamfer_batched (views of one model
    share one GT copy, whose gradient sums over them).  The per-pair fp32 / fp64 rule is chamfer_batched's.  The clouds
    are packed with torch.cat, so autograd carries the packed gradient of dpc_nearest_batched_bwd back to the inputs.
    No host synchronisation and no finiteness check: a NaN or inf coordinate gives non-finite output, as in torch.  The
    values equal chamfer_batched's bit for bit (without squared).  Where a point coincides with its nearest neighbour the
    gradient of the distance is defined as zero (the reference's autograd: NaN); see include/dpc_render.h.  An empty GT
    for a non-empty prediction raises ValueError."""
    P_list, G_list = _loss_clouds(preds, "preds"), _loss_clouds(gts, "gts")
    P = len(P_list)
    if gt_of is None:
        if len(G_list) != P:
            raise ValueError("chamfer_loss: %d predictions and %d GT clouds need gt_of" % (P, len(G_list)))
        gt_of = range(P)
    gt_of = list(gt_of)
    if len(gt_of) != P or any(not isinstance(k, (int, np.integer)) or k < 0 or k >= len(G_list) for k in gt_of):
        raise ValueError("chamfer_loss: gt_of must map each of the %d predictions to one of %d GT clouds" % (P, len(G_list)))
    gt_of = [int(k) for k in gt_of]
    for i, k in enumerate(gt_of):
        if len(G_list[k]) == 0 and len(P_list[i]) > 0:
            raise ValueError("chamfer_loss: GT cloud %d is empty but prediction %d is not (argmin of an empty set)" % (k, i))
    dev = _batch.device(_WHAT, P_list, G_list)
    if P == 0:
        return torch.empty((0, 2), dtype=torch.float64, device=dev)
    f64 = [P_list[i].dtype == torch.float64 or G_list[k].dtype == torch.float64 for i, k in enumerate(gt_of)]
    rows, order = [], []
    for want in (False, True):
        sel = [i for i in range(P) if f64[i] == want]
        if not sel:
            continue
        dtype = torch.float64 if want else torch.float32
        used = sorted({gt_of[i] for i in sel})
        clouds = [G_list[k] for k in used] + [P_list[i] for i in sel]
        start = np.cumsum([0] + [len(c) for c in clouds])
        if start[-1] > _batch.INT32_MAX:
            raise ValueError("chamfer_loss: more than 2^31 - 1 points in one call")
        slot = {k: j for j, k in enumerate(used)}
        desc = np.zeros((2 * len(sel), 4), dtype=np.int64)
        for j, i in enumerate(sel):
            ps, pn = start[len(used) + j], len(P_list[i])
            gs, gn = start[slot[gt_of[i]]], len(G_list[gt_of[i]])
            desc[2 * j] = (ps, pn, gs, gn)
            desc[2 * j + 1] = (gs, gn, ps, pn)
        packed = torch.cat([c.to(device=dev, dtype=dtype) for c in clouds])
        rows.append(nearest_batched(packed, desc, squared=squared).view(len(sel), 2))
        order += sel
    if len(rows) == 1:
        return rows[0]
    inverse = np.argsort(np.asarray(order))
    return torch.cat(rows)[torch.from_numpy(inverse).to(dev)]


def chamfer_of_split(predictions, gt_clouds, reference_rotation=None, models_per_call=256):
    """The reference's chamfer_dists (eval_chamfer_to.py:95-136) for M models: [M,V,2] float64 numpy, bit for bit.

    predictions: per model (points [V,N,3], num_points [V] | None) -- or load_predictions' (points, camera_pose,
    num_points); view i is truncated to its first num_points[i] points (:111-113).  gt_clouds: per model [n,3].
    reference_rotation: a [1,4] quaternion (float64 as loadmat gives it) applied to every view first, the result kept in the
    promoted dtype (:116-120).  Models go through in groups of models_per_call (bounding device memory); the result does
    not depend on the grouping.  Every argument is checked before anything is launched."""
    split = _split.Split("chamfer_of_split", predictions, gt_clouds, reference_rotation, models_per_call, refuse_empty_gt=True)
    out = np.zeros((split.M, split.V, 2), dtype=np.float64)
    if split.empty:
        return out
    dev = _batch.device(_WHAT, *split.tensors())
    for group in split.groups:
        views_list, gt_of = split.views(group, dev)
        split.store(out, group, chamfer_batched(views_list, [split.gts[m] for m in group], gt_of))
    return out


def eval_chamfer(save_dir, model_names, load_gt, num_views=None, reference_rotation=None, out_name=None, out_dir=None,
                 models_per_call=256):
    """run_eval's loop (eval_chamfer_to.py:88-145) over <save_dir>/<model>_pc.pkl.

    load_gt(model) -> [n,3] GT cloud, or None when it has none (e.g. scipy.io.loadmat(path)["points"]); a model whose
    pickle or GT is missing is skipped, as the reference does.  num_views: views per model (default: all in the pickle).
    Returns {"chamfer": [M',V,2], "model_names": the M' evaluated models, "final": np.mean(chamfer, axis=(0, 1)) * 100}.
    With out_name, writes "chamfer_<out_name>.txt" ("{} {}\\n" of final) into out_dir (default: save_dir's parent, the
    reference's experiment directory).  Models are read and evaluated models_per_call at a time."""
    def load(name, i):
        path = os.path.join(save_dir, "%s_pc.pkl" % name)
        if not os.path.isfile(path):
            return None
        gt = load_gt(name)
        if gt is None:
            return None
        points, _, nums = load_predictions(path)
        if num_views is not None:
            points = points[:num_views]
            nums = None if nums is None else nums[:num_views]
        return (points, nums), gt

    names, chamfer = [], []
    for batch in _split.batches(model_names, load, models_per_call):
        chamfer.append(chamfer_of_split([pred for _, (pred, _) in batch], [gt for _, (_, gt) in batch], reference_rotation,
                                        models_per_call))
        names.extend(name for name, _ in batch)
    V = num_views if num_views is not None else (chamfer[0].shape[1] if chamfer else 0)
    dists = np.concatenate(chamfer) if chamfer else np.zeros((0, V, 2), dtype=np.float64)
    final = np.mean(dists, axis=(0, 1)) * 100
    if out_name is not None:
        out_dir = os.path.dirname(os.path.normpath(save_dir)) if out_dir is None else out_dir
        with open(os.path.join(out_dir, "chamfer_{}.txt".format(out_name)), "w") as f:
            f.write("{} {}\n".format(final[0], final[1]))
    return {"chamfer": dists, "model_names": names, "final": final}
